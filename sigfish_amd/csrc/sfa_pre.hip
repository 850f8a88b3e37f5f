// sfa_pre.hip -- the stages in front of the alignment on the device: raw samples in (event detection,
// query window, normalisation: sfa_align_raw) and BLOW5 records in (inflate, field parsing, StreamVByte: sfa_align_blow5), each
// ending in the alignment stage of sfa_align.hip.
#include "sfa_ctx.hpp"
#include "events_kernels.hpp"
#define SFA_DEFINE_BLOW5_KERNELS
#include "blow5_kernels.hpp"
#include "zstd_kernels.hpp"
#include "host/blow5.hpp"
#include "pre_rules.hpp"

// ---- what both entry points share: the reference's own checks of -p -1 (src/dtw_main.c:263-276), and a query there is something to align with
static int check_window_args(const sfa_ctx_t *c, const char *what, int32_t prefix_size, int32_t query_size) {
    if (prefix_size < 0 && (!(c->flag & SFA_RNA) || (c->flag & (SFA_END | SFA_INV))))
        return fail(SFA_EINVAL, "%s: automatic query start (prefix_size < 0) needs an RNA context without SFA_END or SFA_INV", what);
    if (query_size <= 0) return fail(SFA_EINVAL, "%s: query_size must be positive", what);
    return SFA_OK;
}

// A group context's call: fn(shard, a, b, the offsets of reads [a, b] rebased to 0) for every shard with reads.  The context
// keeps the count of a call that went through (sfa_event_maps splits its rows by the same ranges).
template <typename F>
static int split_over_shards(sfa_ctx_t *c, const int64_t *off, int32_t n, F fn) {
    c->maps.map_n = -1;
    const int grc = sfa::for_each_shard_range(c, n, [&](size_t r, int32_t a, int32_t b) {
        std::vector<int64_t> own(b - a + 1);
        for (int32_t i = a; i <= b; ++i) own[i - a] = off[i] - off[a];
        return fn(c->shards[r], a, b, own.data());
    });
    if (!grc) c->maps.map_n = n;
    return grc;
}

inline sfa::EvArgs ctx::RawSignal::detector_args(int32_t n) const {
    sfa::EvArgs ea{};
    ea.raw = e_raw.as<int16_t>(), ea.raw_off = e_rawoff.as<int64_t>(), ea.scale = e_scale.as<float>();
    ea.sum = e_sum.as<double>(), ea.sumsq = e_sumsq.as<double>();
    ea.t1 = e_t1.as<float>(), ea.t2 = e_t2.as<float>();
    ea.ev_off = e_evoff.as<int64_t>(), ea.ev_start = e_evstart.as<int32_t>(), ea.ev_length = e_evlen.as<float>();
    ea.ev_mean = e_evmean.as<float>(), ea.ev_stdv = e_evstdv.as<float>(), ea.n_events = e_nev.as<int32_t>();
    ea.n_reads = n, ea.seq_flag = e_flag.as<int32_t>(), ea.peak_flag = e_pflag.as<int32_t>();
    return ea;
}

inline sfa::AutoArgs ctx::RawSignal::auto_args(int32_t n) const {
    sfa::AutoArgs aa{};
    aa.raw = e_raw.as<int16_t>(), aa.raw_off = e_rawoff.as<int64_t>(), aa.scale = e_scale.as<float>();
    aa.csum = e_sumsq.as<int64_t>(), aa.tmean = e_t1.as<float>();  // (sums and t-statistics are no longer needed: ev_stats_kernel ran before)
    aa.ev_off = e_evoff.as<int64_t>(), aa.ev_start = e_evstart.as<int32_t>(), aa.n_events = e_nev.as<int32_t>(), aa.n_reads = n;
    aa.start = e_nev.as<int32_t>() + n;  // (the counts' neighbours: one copy brings both back)
    return aa;
}

// which reads the wave-per-read kernels of the event detection are offered (option "ev_parallel")
static bool ev_par_prefix(const sfa_ctx_t *c) { return (c->opt_ev_parallel & 1) != 0; }
// measured: 76 us against 1.5 ms for a 512-read batch, 2.1 ms against 1.3 ms for 16 Ki reads (it does ~1.3x the work of
// the sequential walk, in 64x more waves): used while the batch cannot fill the chip with one read per lane pair
static bool ev_par_peaks(const sfa_ctx_t *c, int32_t n) { return (c->opt_ev_parallel & 2) != 0 && n <= 8192; }

// Event detection of the n reads whose samples, offsets, scaling and event offsets are in c->raw: prefix sums, t-statistics, peak
// picker, event statistics, each read by the wave-per-read kernels where they certify their result (option "ev_parallel") and by
// the sequential ones otherwise.  Launches only.
static void launch_event_detection(sfa_ctx_t *c, int32_t n, hipStream_t sp) {
    sfa::EvArgs ea = c->raw.detector_args(n);
    const sfa::DetectorParams dp = sfa::detector_params((c->flag & SFA_RNA) != 0);
    ea.w1 = dp.w1, ea.w2 = dp.w2;
    ea.thr1 = dp.thr1, ea.thr2 = dp.thr2, ea.peak_height = dp.peak_height;
    ea.use_flags = ev_par_prefix(c) ? 1 : 0;
    ea.use_peak_flags = ev_par_peaks(c, n) ? 1 : 0;
    const dim3 lane_grid((n + 63) / 64), lane_block(64);
    if (ea.use_flags) hipLaunchKernelGGL(sfa::ev_prefix_par_kernel, dim3(n), dim3(64), 0, sp, ea);  // flags what it cannot do exactly
    hipLaunchKernelGGL(sfa::ev_prefix_kernel, lane_grid, lane_block, 0, sp, ea);
    hipLaunchKernelGGL(sfa::ev_tstat_kernel, dim3(n), dim3(256), 0, sp, ea);
    if (ea.use_peak_flags) hipLaunchKernelGGL(sfa::ev_peaks_spec_kernel, dim3(n), dim3(64), 0, sp, ea);  // wave per read, flags what it cannot certify
    hipLaunchKernelGGL(sfa::ev_peaks_kernel, dim3((n + 31) / 32), dim3(64), 0, sp, ea);  // two lanes per read (all reads, or the flagged ones)
    hipLaunchKernelGGL(sfa::ev_stats_kernel, dim3(n), dim3(256), 0, sp, ea);
}

// RNA automatic query start: adaptor, poly-A tail, first event behind it.  Launches only.
static void launch_auto_start(sfa_ctx_t *c, int32_t n, hipStream_t sp) {
    sfa::AutoArgs aa = c->raw.auto_args(n);
    aa.lo = sfa::adaptor_params(c->pore).lo;
    aa.std_scale = sfa::adaptor_params(c->pore).std_scale;
    hipLaunchKernelGGL(sfa::ev_autostart_tmean_kernel, dim3(n), dim3(256), 0, sp, aa);
    hipLaunchKernelGGL(sfa::ev_autostart_scan_kernel, dim3((n + 63) / 64), dim3(64), 0, sp, aa);
}

// The inputs of the event detection into c->raw: the samples (raw == nullptr: they are there already), their offsets, the fp32
// scaling of event_single() and the event offsets (pre_rules.hpp).  ev_off and scale are the caller's: the copies are
// asynchronous, so both live until the caller has synchronised.  `what` names the caller.
static int upload_raw_batch(sfa_ctx_t *c, const char *what, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n,
                            hipStream_t sp, std::vector<int64_t> &ev_off, std::vector<float> &scale) {
    const int64_t total = raw_off[n] - raw_off[0];
    if (total < 0 || raw_off[0] != 0) return fail(SFA_EINVAL, "%s: raw_off must start at 0 and be monotone", what);
    ev_off.resize(n + 1);
    scale.resize(2 * static_cast<size_t>(n));
    ev_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t len = raw_off[i + 1] - raw_off[i];
        if (len < 0) return fail(SFA_EINVAL, "%s: raw_off not monotone at read %d", what, i);
        ev_off[i + 1] = ev_off[i] + sfa::event_capacity(len);
        const sfa::RawScale rs = sfa::raw_scale(scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2]);
        scale[2 * i] = rs.offset;
        scale[2 * i + 1] = rs.unit;
    }
    if (int rc = c->raw.reserve(total, static_cast<size_t>(n), static_cast<size_t>(ev_off[n]))) return rc;
    if (raw) HIP_TRY(hipMemcpyAsync(c->raw.e_raw.p, raw, 2 * (size_t)total, hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->raw.e_rawoff.p, raw_off, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->raw.e_scale.p, scale.data(), 8 * (size_t)n, hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->raw.e_evoff.p, ev_off.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, sp));
    return SFA_OK;
}

// ---- sfa_align_raw, stage by stage (what a stage hands on lies in RawCall) ----

struct RawCall {
    const int16_t *raw;  // nullptr: the samples are already in c->raw.e_raw (decoded on the device, sfa_align_blow5), laid out by raw_off
    const int64_t *raw_off;
    const double *scaling;
    int32_t n, prefix_size, query_size;
    sfa_result_t *rows;
    sfa_query_info_t *info;
    sfa_event_t *query_events;
    std::vector<int64_t> ev_off, qstart, q_off;  // (ev_off and scale: read by asynchronous copies until raw_counts_back has waited)
    std::vector<float> scale;
    bool auto_start() const { return prefix_size < 0; }
};

// upload, event detection, automatic start: everything the host has to wait for before it can plan the windows
static int raw_launch_events(sfa_ctx_t *c, RawCall &k) {
    HIP_TRY(hipSetDevice(c->device));
    if (k.raw) HIP_TRY(hipStreamSynchronize(c->stream));  // (device-resident samples: their decoder is still in flight on this stream)
    hipStream_t sp = c->stream;
    if (int rc = upload_raw_batch(c, "sfa_align_raw", k.raw, k.raw_off, k.scaling, k.n, sp, k.ev_off, k.scale)) return rc;
    HIP_TRY(hipEventRecord(c->eev[0], sp));
    launch_event_detection(c, k.n, sp);
    if (k.auto_start()) launch_auto_start(c, k.n, sp);
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(c->eev[1], sp));
    return SFA_OK;
}

// event counts (and automatic starts behind them) into page-locked memory, which later takes the three raw-coordinate columns
static int raw_counts_back(sfa_ctx_t *c, const RawCall &k) {
    if (int rc = c->io.h_small.reserve(16 * (size_t)k.n)) return rc;
    HIP_TRY(hipMemcpyAsync(c->io.h_small.p, c->raw.e_nev.p, (k.auto_start() ? 8 : 4) * (size_t)k.n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SFA_OK;
}

// query windows on the host (query_window, pre_rules.hpp); the arithmetic part runs on the device
static void raw_plan_windows(const sfa_ctx_t *c, RawCall &k) {
    const int32_t *nev = c->io.h_small.as<int32_t>(), *auto_st = nev + k.n;
    k.qstart.assign(k.n, 0);
    k.q_off.assign(k.n + 1, 0);
    for (int32_t i = 0; i < k.n; ++i) {
        const sfa::QueryWindow w = sfa::query_window(nev[i], k.raw_off[i + 1] - k.raw_off[i], k.prefix_size, k.query_size, (c->flag & SFA_END) != 0,
                                                     k.auto_start(), k.auto_start() ? auto_st[i] : -1);
        k.qstart[i] = w.start;
        k.q_off[i + 1] = k.q_off[i] + (w.end - w.start);
        k.info[i].n_events = nev[i];
        k.info[i].qstart = w.start, k.info[i].qend = w.end;
        k.info[i].status = w.status, k.info[i].pad = 0;
    }
}

// normalised queries, raw-coordinate bounds and (for SAM output on the host) the query windows' event tables
static int raw_build_queries(sfa_ctx_t *c, const RawCall &k) {
    const int32_t n = k.n;
    const ctx::RawSignal &r = c->raw;
    hipStream_t st = c->stream;
    if (int rc = c->io.reserve(k.q_off[n], static_cast<size_t>(n))) return rc;
    HIP_TRY(hipMemcpyAsync(r.e_qstart.p, k.qstart.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(r.e_qoff.p, k.q_off.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->eev[2], st));
    sfa::QueryArgs qa{r.e_evmean.as<float>(), r.e_evoff.as<int64_t>(), r.e_qstart.as<int64_t>(), r.e_qoff.as<int64_t>(), c->io.d_queries.as<float>(), n};
    hipLaunchKernelGGL(sfa::ev_query_kernel, dim3(n), dim3(64), 0, st, qa);  // one wave per read
    sfa::BoundsArgs ba{r.e_evstart.as<int32_t>(), r.e_evlen.as<float>(), r.e_evoff.as<int64_t>(), r.e_qstart.as<int64_t>(),
                       r.e_qoff.as<int64_t>(), r.e_b0.as<int32_t>(), r.e_b1.as<int32_t>(), r.e_b2.as<float>(), n};
    hipLaunchKernelGGL(sfa::ev_bounds_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ba);
    if (k.query_events) {
        static_assert(sizeof(sfa_event_t) == 24, "event record layout");
        const size_t qe_bytes = sizeof(sfa_event_t) * static_cast<size_t>(n) * static_cast<size_t>(k.query_size);
        if (int rc = c->raw.e_qev.reserve(qe_bytes)) return rc;
        sfa::PackArgs pa{r.e_evstart.as<int32_t>(), r.e_evlen.as<float>(), r.e_evstdv.as<float>(), r.e_evoff.as<int64_t>(),
                         r.e_qstart.as<int64_t>(), r.e_qoff.as<int64_t>(), c->io.d_queries.as<float>(), r.e_qev.as<uint64_t>(), k.query_size};
        hipLaunchKernelGGL(sfa::ev_pack_events_kernel, dim3(n), dim3(128), 0, st, pa);
        HIP_TRY(hipMemcpyAsync(k.query_events, r.e_qev.p, qe_bytes, hipMemcpyDeviceToHost, st));
    }
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(c->eev[3], st));
    c->raw.eev_pending = true;
    return SFA_OK;
}

// rows and the raw coordinates of every alignment into the caller's arrays
static int raw_collect(sfa_ctx_t *c, const RawCall &k) {
    const size_t n = static_cast<size_t>(k.n);
    hipStream_t st = c->stream;
    int32_t *b0 = c->io.h_small.as<int32_t>(), *b1 = b0 + n;
    float *b2 = reinterpret_cast<float *>(b1 + n);
    HIP_TRY(hipMemcpyAsync(c->io.h_out.p, c->io.d_out.p, sizeof(sfa_result_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b0, c->raw.e_b0.p, 4 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b1, c->raw.e_b1.p, 4 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b2, c->raw.e_b2.p, 4 * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(k.rows, c->io.h_out.p, sizeof(sfa_result_t) * n);
    for (size_t i = 0; i < n; ++i) {
        k.info[i].start_raw_idx = static_cast<uint64_t>(b0[i]);
        k.info[i].end_raw_idx = static_cast<uint64_t>(static_cast<float>(static_cast<uint64_t>(b1[i])) + b2[i]);  // u64 + float, as in C
    }
    return sfa::resolve_profile(c);
}

static int align_raw_impl(sfa_ctx_t *c, RawCall k) {
    if (int rc = check_window_args(c, "sfa_align_raw", k.prefix_size, k.query_size)) return rc;
    if (k.n == 0) return SFA_OK;
    if (!c->shards.empty())
        return split_over_shards(c, k.raw_off, k.n, [&](sfa_ctx_t *shard, int32_t a, int32_t b, const int64_t *off) {
            if (!k.raw) return fail(SFA_EINVAL, "sfa_align_raw: device-resident samples need a single-device context");
            return sfa_align_raw_ex(shard, k.raw + k.raw_off[a], off, k.scaling + 3 * static_cast<size_t>(a), b - a, k.prefix_size, k.query_size,
                                    k.rows + a, k.info + a,
                                    k.query_events ? k.query_events + static_cast<size_t>(a) * static_cast<size_t>(k.query_size) : nullptr);
        });
    if (int rc = raw_launch_events(c, k)) return rc;
    if (int rc = raw_counts_back(c, k)) return rc;
    raw_plan_windows(c, k);
    if (int rc = raw_build_queries(c, k)) return rc;
    // the queries must be complete before align_device's uploads reuse the pinned staging area; same stream, in order
    if (int rc = sfa::align_device(c, c->io.d_queries.as<float>(), k.q_off.data(), k.n, c->io.d_out.as<sfa::ResultRow>())) return rc;
    return raw_collect(c, k);
}

// ---- sfa_align_blow5, stage by stage (what a stage hands on lies in Blow5Call) ----

struct Blow5Call {
    const uint8_t *records;
    const int64_t *rec_off;
    int32_t n, record_zlib, signal_svb;
    sfa_read_head_t *heads;
    sfa::FieldsArgs fa;
    std::vector<int64_t> slot;     // [n + 1] where every record inflates to (read by an asynchronous copy until blow5_heads_back has waited)
    std::vector<int64_t> raw_off;  // [n + 1] samples of every read, and their
    std::vector<double> scaling;   // [n][3] digitisation, offset, range: the arguments of the raw path
    std::vector<int16_t> raw;      // the host reader's samples (the device route leaves them on the device)
    std::vector<int32_t> status;   // [n] what the device stages made of every record: 0 decoded, or one of kRec* (include/sigfish_amd.h)
    std::vector<int64_t> zoff;     // zstd records: [n + 1] where every decoder's scratch area starts (read by an asynchronous copy, as slot is)
};
constexpr int kDeclined = 1;  // a device route's answer beside SFA_OK and errors: the host reader takes the batch (sfa_last_error() says why)
constexpr int32_t kRecInflate = SFA_BLOW5_INFLATE, kRecFields = SFA_BLOW5_FIELDS, kRecStream = SFA_BLOW5_STREAM;
constexpr int64_t kMaxSampleTotal = INT64_MAX / 2;  // samples of a batch: their bytes are still an int64_t

static bool any_declined(const Blow5Call &k) {
    for (int32_t st : k.status)
        if (st != 0) return true;
    return false;
}

// records per wave of the device inflate: about one wave per SIMD (blow5_inflate_kernel)
static int inflate_lanes(int32_t n, int cu_count) {
    const int64_t simds = static_cast<int64_t>(cu_count) * 4;
    int lanes = 1;
    while (lanes < sfa::kInfMaxLanes && static_cast<int64_t>(n) > simds * lanes) lanes *= 2;
    return lanes;
}

// one read's head and its three doubles of the raw path's scaling, from wherever the record was parsed; dor: digitisation, offset, range
static void fill_head(sfa_read_head_t &h, double *scaling, const void *id, int32_t id_len, int64_t n_samples, const void *dor, int64_t record_bytes) {
    memcpy(h.read_id, id, id_len);
    h.read_id[id_len] = 0;
    h.id_len = id_len;
    h.n_samples = n_samples;
    memcpy(scaling, dor, 24);
    h.digitisation = scaling[0], h.offset = scaling[1], h.range = scaling[2];
    h.record_bytes = record_bytes;
}

// records up, decompressed (zlib: blow5_inflate_kernel, zstd: blow5_zstd_kernel) and their fields parsed into head rows: launches only
static int blow5_launch_fields(sfa_ctx_t *c, Blow5Call &k) {
    const int32_t n = k.n;
    ctx::Blow5 &b = c->blow5;
    hipStream_t sp = c->stream;
    const int64_t in_bytes = k.rec_off[n];
    // a compressed record inflates into a slot of 4x its size + 4 KB (svb-zd signals deflate by ~1.5x; a record that needs
    // more is handed to the host reader with the rest of the batch)
    std::vector<int64_t> &slot = k.slot;
    for (int32_t i = 0; i < n; ++i) slot[i + 1] = slot[i] + (k.record_zlib ? (((k.rec_off[i + 1] - k.rec_off[i]) * 4 + 4096 + 15) & ~int64_t(15)) : 0);
    // zstd records: every decoder's tables and the literals of a block (at most the slot, at most 128 KB) in an area of its own
    const bool zstd = k.record_zlib == SFA_PRESS_ZSTD;
    std::vector<int64_t> &zoff = k.zoff;
    zoff.assign(zstd ? n + 1 : 0, 0);
    for (int32_t i = 0; zstd && i < n; ++i) zoff[i + 1] = zoff[i] + sfa::blow5_zstd_scratch_bytes(slot[i + 1] - slot[i]);
    if (int rc = b.reserve(static_cast<size_t>(in_bytes), k.record_zlib ? slot[n] : -1, static_cast<size_t>(n), sfa::kBlow5HeadBytes, zstd ? zoff[n] : 0)) return rc;
    HIP_TRY(hipMemcpyAsync(b.b_in.p, k.records, static_cast<size_t>(in_bytes), hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(b.b_inoff.p, k.rec_off, 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemsetAsync(b.b_bad.p, 0, 4 * static_cast<size_t>(n), sp));
    HIP_TRY(hipEventRecord(c->bev[0], sp));
    if (zstd) {
        HIP_TRY(hipMemcpyAsync(b.b_outoff.p, slot.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
        HIP_TRY(hipMemcpyAsync(b.b_zoff.p, zoff.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
        sfa::launch_blow5_zstd(sfa::ZstdArgs{b.b_in.as<uint8_t>(), b.b_inoff.as<int64_t>(), b.b_out.as<uint8_t>(), b.b_outoff.as<int64_t>(), b.b_len.as<int32_t>(),
                                             b.b_zscratch.as<uint8_t>(), b.b_zoff.as<int64_t>(), n},
                               c->cu_count, c->opt_zstd_tables == 1, sp);
        KERNEL_TRY();
    } else if (k.record_zlib) {
        HIP_TRY(hipMemcpyAsync(b.b_outoff.p, slot.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
        sfa::InflateArgs ia{b.b_in.as<uint8_t>(), b.b_inoff.as<int64_t>(), b.b_out.as<uint8_t>(), b.b_outoff.as<int64_t>(), b.b_len.as<int32_t>(), n};
        const int lanes = inflate_lanes(n, c->cu_count);
        hipLaunchKernelGGL(sfa::blow5_inflate_kernel, dim3((n + lanes - 1) / lanes), dim3(64), sizeof(sfa::InflateLds) * lanes, sp, ia, lanes);
        KERNEL_TRY();
    }
    const bool z = k.record_zlib != 0;  // the payloads: inflated, or the records themselves
    k.fa = sfa::FieldsArgs{(z ? b.b_out : b.b_in).as<uint8_t>(), (z ? b.b_outoff : b.b_inoff).as<int64_t>(), z ? b.b_len.as<int32_t>() : nullptr,
                           b.b_head.as<uint8_t>(), k.signal_svb ? 1 : 0, n};
    hipLaunchKernelGGL(sfa::blow5_fields_kernel, dim3((n + 63) / 64), dim3(64), 0, sp, k.fa);
    KERNEL_TRY();
    return SFA_OK;
}

// the head rows back and into the caller's heads, every record's verdict into k.status.  A record the device declined counts no
// samples (blow5_svb_kernel leaves out whatever its slot does not match) and leaves an empty head; the first one's reason is
// kept in sfa_last_error() for whoever wants to know why.  Behind the parser's own checks, the host takes no count on trust:
// not one beyond what the record's bytes can hold, not a total whose bytes would leave int64_t.
static int blow5_heads_back(sfa_ctx_t *c, Blow5Call &k) {
    const int32_t n = k.n;
    const uint8_t *hh = c->blow5.h_head.as<uint8_t>();
    // (behind the rows: n words for blow5_decode_signals' flags, then n for the inflated lengths)
    const int32_t *inflated = reinterpret_cast<const int32_t *>(hh + static_cast<size_t>(n) * sfa::kBlow5HeadBytes) + n;
    HIP_TRY(hipMemcpyAsync(c->blow5.h_head.p, c->blow5.b_head.p, static_cast<size_t>(n) * sfa::kBlow5HeadBytes, hipMemcpyDeviceToHost, c->stream));
    if (k.record_zlib) HIP_TRY(hipMemcpyAsync(const_cast<int32_t *>(inflated), c->blow5.b_len.p, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    bool said = false;
    for (int32_t i = 0; i < n; ++i) {
        const uint8_t *h = hh + static_cast<size_t>(i) * sfa::kBlow5HeadBytes;
        int32_t status, id_len;
        int64_t ns;
        memcpy(&status, h + sfa::kHeadStatus, 4);
        memcpy(&id_len, h + sfa::kHeadIdLen, 4);
        memcpy(&ns, h + sfa::kHeadSamples, 8);
        const int64_t bytes = k.rec_off[i + 1] - k.rec_off[i];
        const int64_t payload = k.record_zlib ? inflated[i] : bytes;
        // a plain sample takes two bytes, four svb-zd samples at least their key byte
        const int64_t room = k.signal_svb ? 4 * std::max<int64_t>(payload, 0) : payload / 2;
        int32_t verdict = 0;
        if (k.record_zlib && inflated[i] < 0)
            verdict = kRecInflate;
        else if (status != 0 || id_len < 0 || id_len > static_cast<int32_t>(sizeof(k.heads[i].read_id)) - 1 || ns < 0 || ns > room || ns > kMaxSampleTotal - k.raw_off[i])
            verdict = kRecFields;
        k.status[i] = verdict;
        if (verdict != 0) {
            if (!said)
                (void)fail(SFA_OK, "sfa_align_blow5: device declined record %d (status %d, id of %d bytes, %lld samples): host reader takes the batch", i,
                           status, id_len, static_cast<long long>(ns));
            said = true;
            memset(&k.heads[i], 0, sizeof k.heads[i]);
            k.heads[i].record_bytes = bytes;
            k.raw_off[i + 1] = k.raw_off[i];
            continue;
        }
        fill_head(k.heads[i], &k.scaling[3 * static_cast<size_t>(i)], h + sfa::kHeadId, id_len, ns, h + sfa::kHeadScaling, bytes);
        k.raw_off[i + 1] = k.raw_off[i] + ns;
    }
    return SFA_OK;
}

// the signals into c->raw.e_raw, where the raw path takes them from; a signal whose data stream is longer or shorter than its keys
// say gets kRecStream in k.status (its samples are then not to be used)
static int blow5_decode_signals(sfa_ctx_t *c, Blow5Call &k) {
    const int32_t n = k.n;
    hipStream_t sp = c->stream;
    if (int rc = c->raw.reserve_samples(k.raw_off[n], static_cast<size_t>(n))) return rc;
    HIP_TRY(hipMemcpyAsync(c->raw.e_rawoff.p, k.raw_off.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
    sfa::SvbArgs sa{k.fa.payload, k.fa.payload_off, c->blow5.b_head.as<uint8_t>(), c->raw.e_rawoff.as<int64_t>(), c->raw.e_raw.as<int16_t>(),
                    c->blow5.b_bad.as<int32_t>(), k.signal_svb ? 1 : 0, n};
    hipLaunchKernelGGL(sfa::blow5_svb_kernel, dim3((n + 3) / 4), dim3(256), 0, sp, sa);
    KERNEL_TRY();
    int32_t *bad = reinterpret_cast<int32_t *>(c->blow5.h_head.as<uint8_t>() + static_cast<size_t>(n) * sfa::kBlow5HeadBytes);
    HIP_TRY(hipMemcpyAsync(bad, c->blow5.b_bad.p, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, sp));
    HIP_TRY(hipEventRecord(c->bev[1], sp));
    HIP_TRY(hipStreamSynchronize(sp));
    bool said = false;
    for (int32_t i = 0; i < n; ++i)
        if (bad[i] != 0 && k.status[i] == 0) {
            k.status[i] = kRecStream;
            if (!said) (void)fail(SFA_OK, "sfa_align_blow5: signal of record %d is longer or shorter than its keys say: host reader takes the batch", i);
            said = true;
        }
    return SFA_OK;
}

// host reader for the whole batch (own inflate / zlib, SSSE3 StreamVByte): malformed records are reported from here
static int blow5_host_reader(sfa_ctx_t *c, Blow5Call &k) {
    c->prof.blow5_fallbacks = ++c->blow5.blow5_fallbacks;  // (visible at once: a batch the host reader refuses as well resolves no profile)
    for (int32_t i = 0; i < k.n; ++i) {
        sfa::Blow5Record rec;
        std::string err;
        const int64_t bytes = k.rec_off[i + 1] - k.rec_off[i];
        if (!sfa::parse_blow5_record(k.records + k.rec_off[i], static_cast<size_t>(bytes), k.record_zlib, k.signal_svb, &rec, &err))
            return fail(SFA_EINVAL, "sfa_align_blow5: record %d: %s", i, err.c_str());
        if (rec.read_id.size() > sizeof(k.heads[i].read_id) - 1) return fail(SFA_ERANGE, "sfa_align_blow5: record %d: read id of %zu bytes", i, rec.read_id.size());
        const double dor[3] = {rec.digitisation, rec.offset, rec.range};
        fill_head(k.heads[i], &k.scaling[3 * static_cast<size_t>(i)], rec.read_id.data(), static_cast<int32_t>(rec.read_id.size()), static_cast<int64_t>(rec.raw.size()), dor, bytes);
        k.raw.insert(k.raw.end(), rec.raw.begin(), rec.raw.end());
        k.raw_off[i + 1] = static_cast<int64_t>(k.raw.size());
    }
    if (k.raw.empty()) k.raw.push_back(0);
    return SFA_OK;
}

extern "C" {

int sfa_align_raw(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, int32_t prefix_size,
                  int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info) {
    return sfa_align_raw_ex(c, raw, raw_off, scaling, n, prefix_size, query_size, rows, info, nullptr);
}

int sfa_align_raw_ex(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, int32_t prefix_size,
                     int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_event_t *query_events) {
    if (!c || n < 0 || (n > 0 && (!raw || !raw_off || !scaling || !rows || !info))) return fail(SFA_EINVAL, "sfa_align_raw: bad argument");
    return align_raw_impl(c, RawCall{raw, raw_off, scaling, n, prefix_size, query_size, rows, info, query_events});
}

// BLOW5 records in, result rows out: records are decompressed and parsed on the device (blow5_kernels.hpp), then the path of
// sfa_align_raw continues on the samples where they already are -- or, where the device declined, on the host reader's.
int sfa_align_blow5(sfa_ctx_t *c, const uint8_t *records, const int64_t *rec_off, int32_t n, int32_t record_zlib, int32_t signal_svb,
                    int32_t prefix_size, int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_read_head_t *heads,
                    sfa_event_t *query_events) {
    if (!c || n < 0 || (n > 0 && (!records || !rec_off || !rows || !info || !heads))) return fail(SFA_EINVAL, "sfa_align_blow5: bad argument");
    if (int rc = check_window_args(c, "sfa_align_blow5", prefix_size, query_size)) return rc;
    if (n == 0) return SFA_OK;
    if (!c->shards.empty())
        return split_over_shards(c, rec_off, n, [&](sfa_ctx_t *shard, int32_t a, int32_t b, const int64_t *off) {
            return sfa_align_blow5(shard, records + rec_off[a], off, b - a, record_zlib, signal_svb, prefix_size, query_size, rows + a, info + a, heads + a,
                                   query_events ? query_events + static_cast<size_t>(a) * static_cast<size_t>(query_size) : nullptr);
        });
    if (rec_off[0] != 0) return fail(SFA_EINVAL, "sfa_align_blow5: rec_off must start at 0");
    for (int32_t i = 0; i < n; ++i)
        if (rec_off[i + 1] < rec_off[i]) return fail(SFA_EINVAL, "sfa_align_blow5: rec_off not monotone at record %d", i);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    Blow5Call k{records, rec_off, n, record_zlib, signal_svb, heads, {}, std::vector<int64_t>(n + 1, 0), std::vector<int64_t>(n + 1, 0), std::vector<double>(3 * static_cast<size_t>(n)), {}, std::vector<int32_t>(n, 0)};
    // one declined record and the host reader takes the batch: the signals are not even launched behind declined fields
    int rc = blow5_launch_fields(c, k);
    if (!rc) rc = blow5_heads_back(c, k);
    if (!rc && any_declined(k)) rc = kDeclined;
    if (!rc) rc = blow5_decode_signals(c, k);
    if (!rc && any_declined(k)) rc = kDeclined;
    if (!rc) c->blow5.bev_pending = true;
    if (rc == kDeclined) rc = blow5_host_reader(c, k);  // the one place where a batch changes routes
    if (rc) return rc;
    return align_raw_impl(c, RawCall{k.raw.empty() ? nullptr : k.raw.data(), k.raw_off.data(), k.scaling.data(), n, prefix_size, query_size, rows, info, query_events});
}

// (testing hook of the device-side record decoder: the stages of sfa_align_blow5 above and what they left on the device, no host
// reader behind them; see include/sigfish_amd.h)
int sfa_decode_blow5_device(sfa_ctx_t *c, const uint8_t *records, const int64_t *rec_off, int32_t n, int32_t record_zlib, int32_t signal_svb,
                            int32_t *status, sfa_read_head_t *heads, int64_t *raw_off, int16_t *samples, int64_t capacity) {
    if (!c || !c->shards.empty() || n < 0 || capacity < 0 || (n > 0 && (!records || !rec_off || !status || !heads || !raw_off || (capacity > 0 && !samples))))
        return fail(SFA_EINVAL, "sfa_decode_blow5_device: bad argument (single-device context needed)");
    if (n == 0) return SFA_OK;
    if (rec_off[0] != 0) return fail(SFA_EINVAL, "sfa_decode_blow5_device: rec_off must start at 0");
    for (int32_t i = 0; i < n; ++i)
        if (rec_off[i + 1] < rec_off[i]) return fail(SFA_EINVAL, "sfa_decode_blow5_device: rec_off not monotone at record %d", i);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    Blow5Call k{records, rec_off, n, record_zlib, signal_svb, heads, {}, std::vector<int64_t>(n + 1, 0), std::vector<int64_t>(n + 1, 0), std::vector<double>(3 * static_cast<size_t>(n)), {}, std::vector<int32_t>(n, 0)};
    if (int rc = blow5_launch_fields(c, k)) return rc;
    if (int rc = blow5_heads_back(c, k)) return rc;
    memcpy(raw_off, k.raw_off.data(), 8 * static_cast<size_t>(n + 1));
    memcpy(status, k.status.data(), 4 * static_cast<size_t>(n));
    if (k.raw_off[n] > capacity) return fail(SFA_ERANGE, "sfa_decode_blow5_device: %lld samples, room for %lld", static_cast<long long>(k.raw_off[n]), static_cast<long long>(capacity));
    if (int rc = blow5_decode_signals(c, k)) return rc;
    memcpy(status, k.status.data(), 4 * static_cast<size_t>(n));
    if (k.raw_off[n] > 0) HIP_TRY(hipMemcpyAsync(samples, c->raw.e_raw.p, 2 * static_cast<size_t>(k.raw_off[n]), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return SFA_OK;
}

// (testing hook of the device-side inflate alone: n zlib streams in, their bytes out; see include/sigfish_amd.h)
int sfa_inflate_zlib_device(sfa_ctx_t *c, const uint8_t *in, const int64_t *in_off, int32_t n, uint8_t *out, const int64_t *out_off, int32_t *out_len) {
    if (!c || !c->shards.empty() || n < 0 || (n > 0 && (!in || !in_off || !out || !out_off || !out_len)))
        return fail(SFA_EINVAL, "sfa_inflate_zlib_device: bad argument (single-device context needed)");
    if (n == 0) return SFA_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    int rc;
    if ((rc = c->blow5.reserve_inflate(static_cast<size_t>(in_off[n]), out_off[n], static_cast<size_t>(n)))) return rc;
    HIP_TRY(hipMemcpyAsync(c->blow5.b_in.p, in, static_cast<size_t>(in_off[n]), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->blow5.b_inoff.p, in_off, 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->blow5.b_outoff.p, out_off, 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, st));
    sfa::InflateArgs ia{c->blow5.b_in.as<uint8_t>(), c->blow5.b_inoff.as<int64_t>(), c->blow5.b_out.as<uint8_t>(), c->blow5.b_outoff.as<int64_t>(), c->blow5.b_len.as<int32_t>(), n};
    const int lanes = inflate_lanes(n, c->cu_count);
    hipLaunchKernelGGL(sfa::blow5_inflate_kernel, dim3((n + lanes - 1) / lanes), dim3(64), sizeof(sfa::InflateLds) * lanes, st, ia, lanes);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(out, c->blow5.b_out.p, static_cast<size_t>(out_off[n]), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_len, c->blow5.b_len.p, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SFA_OK;
}

// (testing hook of the device-side zstd decoder alone: n records in, their bytes out; see include/sigfish_amd.h)
int sfa_zstd_device(sfa_ctx_t *c, const uint8_t *in, const int64_t *in_off, int32_t n, uint8_t *out, const int64_t *out_off, int32_t *out_len) {
    if (!c || !c->shards.empty() || n < 0 || (n > 0 && (!in || !in_off || !out || !out_off || !out_len)))
        return fail(SFA_EINVAL, "sfa_zstd_device: bad argument (single-device context needed)");
    if (n == 0) return SFA_OK;
    if (in_off[0] != 0 || out_off[0] != 0) return fail(SFA_EINVAL, "sfa_zstd_device: offsets must start at 0");
    std::vector<int64_t> zoff(n + 1, 0);
    for (int32_t i = 0; i < n; ++i) {
        if (in_off[i + 1] < in_off[i] || out_off[i + 1] < out_off[i]) return fail(SFA_EINVAL, "sfa_zstd_device: offsets not monotone at record %d", i);
        zoff[i + 1] = zoff[i] + sfa::blow5_zstd_scratch_bytes(out_off[i + 1] - out_off[i]);
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    ctx::Blow5 &b = c->blow5;
    if (int rc = b.reserve_inflate(static_cast<size_t>(in_off[n]), out_off[n], static_cast<size_t>(n), zoff[n])) return rc;
    HIP_TRY(hipMemcpyAsync(b.b_in.p, in, static_cast<size_t>(in_off[n]), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.b_inoff.p, in_off, 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.b_outoff.p, out_off, 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b.b_zoff.p, zoff.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, st));
    sfa::launch_blow5_zstd(sfa::ZstdArgs{b.b_in.as<uint8_t>(), b.b_inoff.as<int64_t>(), b.b_out.as<uint8_t>(), b.b_outoff.as<int64_t>(), b.b_len.as<int32_t>(),
                                         b.b_zscratch.as<uint8_t>(), b.b_zoff.as<int64_t>(), n},
                           c->cu_count, c->opt_zstd_tables == 1, st);
    KERNEL_TRY();
    HIP_TRY(hipMemcpyAsync(out, b.b_out.p, static_cast<size_t>(out_off[n]), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_len, b.b_len.p, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SFA_OK;
}

// (testing hook of the event detection alone: every read's whole event table, the route each read took and the two t-statistics;
// see include/sigfish_amd.h)
int sfa_detect_events_device(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, sfa_event_t *events,
                             int32_t *n_events, int32_t *route, float *t_short, float *t_long) {
    if (!c || !c->shards.empty() || n < 0 || (n > 0 && (!raw || !raw_off || !scaling || !events || !n_events || !route)))
        return fail(SFA_EINVAL, "sfa_detect_events_device: bad argument (single-device context needed)");
    if (n == 0) return SFA_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    std::vector<int64_t> ev_off;  // as sfa_align_raw: room for event_capacity() records per read
    std::vector<float> scale;
    int rc;
    if ((rc = upload_raw_batch(c, "sfa_detect_events_device", raw, raw_off, scaling, n, st, ev_off, scale))) return rc;
    const int64_t total = raw_off[n];
    const size_t ev_total = static_cast<size_t>(ev_off[n]);
    launch_event_detection(c, n, st);
    KERNEL_TRY();
    std::vector<int32_t> start(ev_total), seq(n), peak(n);
    std::vector<float> length(ev_total), mean(ev_total), stdv(ev_total);
    HIP_TRY(hipMemcpyAsync(start.data(), c->raw.e_evstart.p, 4 * ev_total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(length.data(), c->raw.e_evlen.p, 4 * ev_total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(mean.data(), c->raw.e_evmean.p, 4 * ev_total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(stdv.data(), c->raw.e_evstdv.p, 4 * ev_total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(n_events, c->raw.e_nev.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    const bool par_prefix = ev_par_prefix(c), par_peaks = ev_par_peaks(c, n);  // (a kernel that did not run left its flags stale)
    if (par_prefix) HIP_TRY(hipMemcpyAsync(seq.data(), c->raw.e_flag.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (par_peaks) HIP_TRY(hipMemcpyAsync(peak.data(), c->raw.e_pflag.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (t_short && total > 0) HIP_TRY(hipMemcpyAsync(t_short, c->raw.e_t1.p, 4 * (size_t)total, hipMemcpyDeviceToHost, st));
    if (t_long && total > 0) HIP_TRY(hipMemcpyAsync(t_long, c->raw.e_t2.p, 4 * (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int32_t i = 0; i < n; ++i) {
        route[i] = ((!par_prefix || seq[i] != 0) ? 1 : 0) | ((!par_peaks || peak[i] != 0) ? 2 : 0);
        const int64_t cap = ev_off[i + 1] - ev_off[i];
        if (n_events[i] < 0 || n_events[i] > cap) return fail(SFA_EKERNEL, "sfa_detect_events_device: read %d reports %d events, room for %lld", i, n_events[i], (long long)cap);
        for (int64_t e = 0; e < n_events[i]; ++e) {
            const size_t k = static_cast<size_t>(ev_off[i] + e);
            sfa_event_t rec;
            memset(&rec, 0, sizeof rec);
            rec.start = static_cast<uint64_t>(start[k]);
            rec.length = length[k];
            rec.mean = mean[k];
            rec.stdv = stdv[k];
            events[k] = rec;
        }
    }
    return SFA_OK;
}

}  // extern "C"
