// sfa_pre.hip -- the stages in front of the alignment on the device: raw samples in (event detection,
// query window, normalisation: sfa_align_raw) and BLOW5 records in (inflate, field parsing, StreamVByte: sfa_align_blow5), each
// ending in the alignment stage of sfa_align.hip.
#include "sfa_ctx.hpp"
#include "events_kernels.hpp"
#define SFA_DEFINE_BLOW5_KERNELS
#include "blow5_kernels.hpp"
#include "host/blow5.hpp"

using sfa::ResultRow;
using sfa::resolve_profile;
using sfa::align_device;
using sfa::for_each_shard_range;

extern "C" {

int sfa_align_raw(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, int32_t prefix_size,
                  int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info) {
    return sfa_align_raw_ex(c, raw, raw_off, scaling, n, prefix_size, query_size, rows, info, nullptr);
}

static int align_raw_impl(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, int32_t prefix_size,
                          int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_event_t *query_events);

int sfa_align_raw_ex(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, int32_t prefix_size,
                     int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_event_t *query_events) {
    if (!c || n < 0 || (n > 0 && (!raw || !raw_off || !scaling || !rows || !info))) return fail(SFA_EINVAL, "sfa_align_raw: bad argument");
    return align_raw_impl(c, raw, raw_off, scaling, n, prefix_size, query_size, rows, info, query_events);
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
    const bool rna = (c->flag & SFA_RNA) != 0;
    sfa::EvArgs ea{};
    ea.raw = c->raw.e_raw.as<int16_t>();
    ea.raw_off = c->raw.e_rawoff.as<int64_t>();
    ea.scale = c->raw.e_scale.as<float>();
    ea.sum = c->raw.e_sum.as<double>();
    ea.sumsq = c->raw.e_sumsq.as<double>();
    ea.t1 = c->raw.e_t1.as<float>();
    ea.t2 = c->raw.e_t2.as<float>();
    ea.ev_off = c->raw.e_evoff.as<int64_t>();
    ea.ev_start = c->raw.e_evstart.as<int32_t>();
    ea.ev_length = c->raw.e_evlen.as<float>();
    ea.ev_mean = c->raw.e_evmean.as<float>();
    ea.ev_stdv = c->raw.e_evstdv.as<float>();
    ea.n_events = c->raw.e_nev.as<int32_t>();
    ea.n_reads = n;
    // detector parameters, src/events.c:47-58
    ea.w1 = rna ? 7 : 3;
    ea.w2 = rna ? 14 : 6;
    ea.thr1 = rna ? 2.5f : 1.4f;
    ea.thr2 = 9.0f;
    ea.peak_height = rna ? 1.0f : 0.2f;
    const dim3 lane_grid((n + 63) / 64), lane_block(64);
    ea.seq_flag = c->raw.e_flag.as<int32_t>();
    ea.use_flags = ev_par_prefix(c) ? 1 : 0;
    ea.peak_flag = c->raw.e_pflag.as<int32_t>();
    ea.use_peak_flags = ev_par_peaks(c, n) ? 1 : 0;
    if (ea.use_flags) hipLaunchKernelGGL(sfa::ev_prefix_par_kernel, dim3(n), dim3(64), 0, sp, ea);  // flags what it cannot do exactly
    hipLaunchKernelGGL(sfa::ev_prefix_kernel, lane_grid, lane_block, 0, sp, ea);
    hipLaunchKernelGGL(sfa::ev_tstat_kernel, dim3(n), dim3(256), 0, sp, ea);
    if (ea.use_peak_flags) hipLaunchKernelGGL(sfa::ev_peaks_spec_kernel, dim3(n), dim3(64), 0, sp, ea);  // wave per read, flags what it cannot certify
    hipLaunchKernelGGL(sfa::ev_peaks_kernel, dim3((n + 31) / 32), dim3(64), 0, sp, ea);  // two lanes per read (all reads, or the flagged ones)
    hipLaunchKernelGGL(sfa::ev_stats_kernel, dim3(n), dim3(256), 0, sp, ea);
}

// The inputs of the event detection into c->raw: the samples (raw == nullptr: they are there already), their offsets, the fp32
// scaling of event_single() (src/sigfish.c:343) and the event offsets.  ev_off and scale are the caller's: the copies are
// asynchronous, so both live until the caller has synchronised.  `what` names the caller.
static int upload_raw_batch(sfa_ctx_t *c, const char *what, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n,
                            hipStream_t sp, std::vector<int64_t> &ev_off, std::vector<float> &scale) {
    const int64_t total = raw_off[n] - raw_off[0];
    if (total < 0 || raw_off[0] != 0) return fail(SFA_EINVAL, "%s: raw_off must start at 0 and be monotone", what);
    // event capacity per read: every sample can close at most one event per detector, each detector at most every
    // second sample -> n samples bound the count
    ev_off.resize(n + 1);
    scale.resize(2 * static_cast<size_t>(n));
    ev_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t len = raw_off[i + 1] - raw_off[i];
        if (len < 0) return fail(SFA_EINVAL, "%s: raw_off not monotone at read %d", what, i);
        ev_off[i + 1] = ev_off[i] + len + 2;
        const float range = static_cast<float>(scaling[3 * i + 2]), dig = static_cast<float>(scaling[3 * i]);
        scale[2 * i] = static_cast<float>(scaling[3 * i + 1]);
        scale[2 * i + 1] = range / dig;  // event_single(), src/sigfish.c:343
    }
    if (int rc = c->raw.reserve(total, static_cast<size_t>(n), static_cast<size_t>(ev_off[n]))) return rc;
    if (raw) HIP_TRY(hipMemcpyAsync(c->raw.e_raw.p, raw, 2 * (size_t)total, hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->raw.e_rawoff.p, raw_off, 8 * (size_t)(n + 1), hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->raw.e_scale.p, scale.data(), 8 * (size_t)n, hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->raw.e_evoff.p, ev_off.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, sp));
    return SFA_OK;
}

// raw == nullptr: the samples are already in c->raw.e_raw (decoded on the device, sfa_align_blow5), laid out by raw_off
static int align_raw_impl(sfa_ctx_t *c, const int16_t *raw, const int64_t *raw_off, const double *scaling, int32_t n, int32_t prefix_size,
                          int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_event_t *query_events) {
    // the reference's own checks of -p -1 (src/dtw_main.c:263-276)
    if (prefix_size < 0 && (!(c->flag & SFA_RNA) || (c->flag & (SFA_END | SFA_INV))))
        return fail(SFA_EINVAL, "sfa_align_raw: automatic query start (prefix_size < 0) needs an RNA context without SFA_END or SFA_INV");
    if (query_size <= 0) return fail(SFA_EINVAL, "sfa_align_raw: query_size must be positive");
    if (n == 0) return SFA_OK;
    if (!c->shards.empty()) {
        c->maps.map_n = -1;
        const int grc = for_each_shard_range(c, n, [&](size_t r, int32_t a, int32_t b) {
            std::vector<int64_t> off(b - a + 1);  // the shard's sample offsets start at 0
            for (int32_t i = a; i <= b; ++i) off[i - a] = raw_off[i] - raw_off[a];
            if (!raw) return fail(SFA_EINVAL, "sfa_align_raw: device-resident samples need a single-device context");
            return sfa_align_raw_ex(c->shards[r], raw + raw_off[a], off.data(), scaling + 3 * static_cast<size_t>(a), b - a, prefix_size,
                                    query_size, rows + a, info + a,
                                    query_events ? query_events + static_cast<size_t>(a) * static_cast<size_t>(query_size) : nullptr);
        });
        if (!grc) c->maps.map_n = n;  // (sfa_event_maps splits its rows by the same ranges)
        return grc;
    }
    HIP_TRY(hipSetDevice(c->device));
    if (raw) HIP_TRY(hipStreamSynchronize(c->stream));  // (device-resident samples: their decoder is still in flight on this stream)
    hipStream_t st = c->stream, sp = st;
    std::vector<int64_t> ev_off;
    std::vector<float> scale;
    int rc;
    if ((rc = upload_raw_batch(c, "sfa_align_raw", raw, raw_off, scaling, n, sp, ev_off, scale))) return rc;
    HIP_TRY(hipEventRecord(c->eev[0], sp));
    launch_event_detection(c, n, sp);
    // RNA automatic query start: adaptor, poly-A tail, first event behind it; e_nev[n + i] (the counts' neighbours, one copy)
    const bool auto_start = prefix_size < 0;
    if (auto_start) {
        const dim3 lane_grid((n + 63) / 64), lane_block(64);
        sfa::AutoArgs aa{};
        aa.raw = c->raw.e_raw.as<int16_t>();
        aa.raw_off = c->raw.e_rawoff.as<int64_t>();
        aa.scale = c->raw.e_scale.as<float>();
        aa.csum = c->raw.e_sumsq.as<int64_t>();  // (sums and t-statistics are no longer needed: ev_stats_kernel ran before)
        aa.tmean = c->raw.e_t1.as<float>();
        aa.ev_off = c->raw.e_evoff.as<int64_t>();
        aa.ev_start = c->raw.e_evstart.as<int32_t>();
        aa.n_events = c->raw.e_nev.as<int32_t>();
        aa.start = c->raw.e_nev.as<int32_t>() + n;
        aa.n_reads = n;
        aa.lo = c->pore == 2 ? 500 : 2000;  // JNNV2_RNA_RNA004_ADAPTOR / JNNV2_RNA_R9_ADAPTOR, src/jnn.h
        aa.std_scale = c->pore == 2 ? 0.7f : 0.5f;
        hipLaunchKernelGGL(sfa::ev_autostart_tmean_kernel, dim3(n), dim3(256), 0, sp, aa);
        hipLaunchKernelGGL(sfa::ev_autostart_scan_kernel, lane_grid, lane_block, 0, sp, aa);
    }
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(c->eev[1], sp));
    // page-locked: event counts and automatic starts, then the three raw-coordinate columns
    if ((rc = c->io.h_small.reserve(16 * (size_t)n))) return rc;
    int32_t *nev = c->io.h_small.as<int32_t>();
    const int32_t *auto_st = nev + n;
    HIP_TRY(hipMemcpyAsync(nev, c->raw.e_nev.p, (auto_start ? 8 : 4) * (size_t)n, hipMemcpyDeviceToHost, sp));
    HIP_TRY(hipStreamSynchronize(sp));

    // query windows on the host (normalise_single, src/sigfish.c:433-480); the arithmetic part runs on the device
    std::vector<int64_t> qstart(n), q_off(n + 1);
    q_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int64_t ne = nev[i];
        int64_t s0 = 0, e0 = 0;
        int status = 0;
        bool keep = ne > 0 && (raw_off[i + 1] - raw_off[i]) > 0;
        if (keep) {
            if (!(c->flag & SFA_END)) {
                s0 = prefix_size;
                if (auto_start) {  // detect_query_start() failed: fall back to 50 events (src/sigfish.c:438-446)
                    s0 = auto_st[i] >= 0 ? auto_st[i] : 50;
                    if (auto_st[i] < 0) status |= 4;
                }
                e0 = s0 + query_size;
                if (s0 + 25 > ne) {
                    s0 = e0 = 0;
                    keep = false;
                    status |= 2;
                } else if (e0 > ne) {
                    e0 = ne;
                    status |= 1;
                }
            } else {
                s0 = ne - prefix_size - query_size;
                e0 = ne - prefix_size;
                if (s0 < 0) {
                    s0 = 0;
                    status |= 1;
                }
                if (e0 < 0) {
                    e0 = 0;
                    keep = false;
                    status |= 2;
                }
            }
        }
        if (!keep) s0 = e0 = 0;
        qstart[i] = s0;
        q_off[i + 1] = q_off[i] + (e0 - s0);
        info[i].n_events = ne;
        info[i].qstart = s0;
        info[i].qend = e0;
        info[i].status = status;
        info[i].pad = 0;
    }
    const int64_t nq = q_off[n];
    if ((rc = c->io.reserve(nq, static_cast<size_t>(n)))) return rc;
    HIP_TRY(hipMemcpyAsync(c->raw.e_qstart.p, qstart.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->raw.e_qoff.p, q_off.data(), 8 * (size_t)(n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->eev[2], st));
    sfa::QueryArgs qa{c->raw.e_evmean.as<float>(), c->raw.e_evoff.as<int64_t>(), c->raw.e_qstart.as<int64_t>(), c->raw.e_qoff.as<int64_t>(),
                      c->io.d_queries.as<float>(), n};
    hipLaunchKernelGGL(sfa::ev_query_kernel, dim3(n), dim3(64), 0, st, qa);  // one wave per read
    sfa::BoundsArgs ba{c->raw.e_evstart.as<int32_t>(), c->raw.e_evlen.as<float>(), c->raw.e_evoff.as<int64_t>(), c->raw.e_qstart.as<int64_t>(),
                       c->raw.e_qoff.as<int64_t>(), c->raw.e_b0.as<int32_t>(), c->raw.e_b1.as<int32_t>(), c->raw.e_b2.as<float>(), n};
    hipLaunchKernelGGL(sfa::ev_bounds_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ba);
    if (query_events) {  // the query windows' event tables, for SAM output on the host
        static_assert(sizeof(sfa_event_t) == 24, "event record layout");
        const size_t qe_bytes = sizeof(sfa_event_t) * static_cast<size_t>(n) * static_cast<size_t>(query_size);
        if ((rc = c->raw.e_qev.reserve(qe_bytes))) return rc;
        sfa::PackArgs pa{c->raw.e_evstart.as<int32_t>(), c->raw.e_evlen.as<float>(), c->raw.e_evstdv.as<float>(), c->raw.e_evoff.as<int64_t>(),
                         c->raw.e_qstart.as<int64_t>(), c->raw.e_qoff.as<int64_t>(), c->io.d_queries.as<float>(), c->raw.e_qev.as<uint64_t>(), query_size};
        hipLaunchKernelGGL(sfa::ev_pack_events_kernel, dim3(n), dim3(128), 0, st, pa);
        HIP_TRY(hipMemcpyAsync(query_events, c->raw.e_qev.p, qe_bytes, hipMemcpyDeviceToHost, st));
    }
    KERNEL_TRY();
    HIP_TRY(hipEventRecord(c->eev[3], st));
    c->raw.eev_pending = true;
    // the queries must be complete before align_device's uploads reuse the pinned staging area; same stream, in order
    if ((rc = align_device(c, c->io.d_queries.as<float>(), q_off.data(), n, c->io.d_out.as<ResultRow>()))) return rc;
    int32_t *b0 = c->io.h_small.as<int32_t>(), *b1 = b0 + n;
    float *b2 = reinterpret_cast<float *>(b1 + n);
    HIP_TRY(hipMemcpyAsync(c->io.h_out.p, c->io.d_out.p, sizeof(sfa_result_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b0, c->raw.e_b0.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b1, c->raw.e_b1.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(b2, c->raw.e_b2.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(rows, c->io.h_out.p, sizeof(sfa_result_t) * (size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        info[i].start_raw_idx = static_cast<uint64_t>(b0[i]);
        info[i].end_raw_idx = static_cast<uint64_t>(static_cast<float>(static_cast<uint64_t>(b1[i])) + b2[i]);  // u64 + float, as in C
    }
    return resolve_profile(c);
}

// records per wave of the device inflate: about one wave per SIMD (blow5_inflate_kernel)
static int inflate_lanes(int32_t n, int cu_count) {
    const int64_t simds = static_cast<int64_t>(cu_count) * 4;
    int lanes = 1;
    while (lanes < sfa::kInfMaxLanes && static_cast<int64_t>(n) > simds * lanes) lanes *= 2;
    return lanes;
}

// BLOW5 records in, result rows out: records are decompressed and parsed on the device (blow5_kernels.hpp), then the path of
// sfa_align_raw continues on the samples where they already are.
int sfa_align_blow5(sfa_ctx_t *c, const uint8_t *records, const int64_t *rec_off, int32_t n, int32_t record_zlib, int32_t signal_svb,
                    int32_t prefix_size, int32_t query_size, sfa_result_t *rows, sfa_query_info_t *info, sfa_read_head_t *heads,
                    sfa_event_t *query_events) {
    if (!c || n < 0 || (n > 0 && (!records || !rec_off || !rows || !info || !heads))) return fail(SFA_EINVAL, "sfa_align_blow5: bad argument");
    if (prefix_size < 0 && (!(c->flag & SFA_RNA) || (c->flag & (SFA_END | SFA_INV))))
        return fail(SFA_EINVAL, "sfa_align_blow5: automatic query start (prefix_size < 0) needs an RNA context without SFA_END or SFA_INV");
    if (query_size <= 0) return fail(SFA_EINVAL, "sfa_align_blow5: query_size must be positive");
    if (n == 0) return SFA_OK;
    if (!c->shards.empty()) {
        c->maps.map_n = -1;
        const int grc = for_each_shard_range(c, n, [&](size_t r, int32_t a, int32_t b) {
            std::vector<int64_t> off(b - a + 1);
            for (int32_t i = a; i <= b; ++i) off[i - a] = rec_off[i] - rec_off[a];
            return sfa_align_blow5(c->shards[r], records + rec_off[a], off.data(), b - a, record_zlib, signal_svb, prefix_size, query_size,
                                   rows + a, info + a, heads + a,
                                   query_events ? query_events + static_cast<size_t>(a) * static_cast<size_t>(query_size) : nullptr);
        });
        if (!grc) c->maps.map_n = n;
        return grc;
    }
    if (rec_off[0] != 0) return fail(SFA_EINVAL, "sfa_align_blow5: rec_off must start at 0");
    for (int32_t i = 0; i < n; ++i)
        if (rec_off[i + 1] < rec_off[i]) return fail(SFA_EINVAL, "sfa_align_blow5: rec_off not monotone at record %d", i);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    hipStream_t st = c->stream;
    const int64_t in_bytes = rec_off[n];
    int rc;
    // a compressed record inflates into a slot of 4x its size + 4 KB (svb-zd signals deflate by ~1.5x; a record that needs
    // more is handed to the host reader with the rest of the batch)
    std::vector<int64_t> slot(n + 1);
    slot[0] = 0;
    for (int32_t i = 0; i < n; ++i) slot[i + 1] = slot[i] + (record_zlib ? (((rec_off[i + 1] - rec_off[i]) * 4 + 4096 + 15) & ~int64_t(15)) : 0);
    if ((rc = c->blow5.reserve(static_cast<size_t>(in_bytes), record_zlib ? slot[n] : -1, static_cast<size_t>(n), sfa::kBlow5HeadBytes))) return rc;
    hipStream_t sp = st;
    HIP_TRY(hipMemcpyAsync(c->blow5.b_in.p, records, static_cast<size_t>(in_bytes), hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemcpyAsync(c->blow5.b_inoff.p, rec_off, 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
    HIP_TRY(hipMemsetAsync(c->blow5.b_bad.p, 0, 4 * static_cast<size_t>(n), sp));
    HIP_TRY(hipEventRecord(c->bev[0], sp));
    sfa::FieldsArgs fa{};
    if (record_zlib) {
        HIP_TRY(hipMemcpyAsync(c->blow5.b_outoff.p, slot.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
        sfa::InflateArgs ia{c->blow5.b_in.as<uint8_t>(), c->blow5.b_inoff.as<int64_t>(), c->blow5.b_out.as<uint8_t>(), c->blow5.b_outoff.as<int64_t>(), c->blow5.b_len.as<int32_t>(), n};
        const int lanes = inflate_lanes(n, c->cu_count);
        hipLaunchKernelGGL(sfa::blow5_inflate_kernel, dim3((n + lanes - 1) / lanes), dim3(64), sizeof(sfa::InflateLds) * lanes, sp, ia, lanes);
        KERNEL_TRY();
        fa.payload = c->blow5.b_out.as<uint8_t>();
        fa.payload_off = c->blow5.b_outoff.as<int64_t>();
        fa.payload_len = c->blow5.b_len.as<int32_t>();
    } else {
        fa.payload = c->blow5.b_in.as<uint8_t>();
        fa.payload_off = c->blow5.b_inoff.as<int64_t>();
        fa.payload_len = nullptr;
    }
    fa.head = c->blow5.b_head.as<uint8_t>();
    fa.signal_svb = signal_svb ? 1 : 0;
    fa.n = n;
    hipLaunchKernelGGL(sfa::blow5_fields_kernel, dim3((n + 63) / 64), dim3(64), 0, sp, fa);
    KERNEL_TRY();
    uint8_t *hh = c->blow5.h_head.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(hh, c->blow5.b_head.p, static_cast<size_t>(n) * sfa::kBlow5HeadBytes, hipMemcpyDeviceToHost, sp));
    HIP_TRY(hipStreamSynchronize(sp));
    // the fields of every record; anything the device declined sends the whole batch to the host reader
    std::vector<int64_t> raw_off(n + 1);
    std::vector<double> scaling(3 * static_cast<size_t>(n));
    raw_off[0] = 0;
    bool fallback = false;
    for (int32_t i = 0; i < n && !fallback; ++i) {
        const uint8_t *h = hh + static_cast<size_t>(i) * sfa::kBlow5HeadBytes;
        int32_t status, id_len;
        int64_t ns;
        memcpy(&status, h, 4);
        memcpy(&id_len, h + 4, 4);
        memcpy(&ns, h + 8, 8);
        if (status != 0 || id_len < 0 || id_len > static_cast<int32_t>(sizeof(heads[i].read_id)) - 1 || ns < 0) {
            (void)fail(SFA_OK, "sfa_align_blow5: device declined record %d (status %d, id of %d bytes, %lld samples): host reader takes the batch", i,
                       status, id_len, static_cast<long long>(ns));  // kept in sfa_last_error() for whoever wants to know why
            fallback = true;
            break;
        }
        memcpy(heads[i].read_id, h + 56, id_len);
        heads[i].read_id[id_len] = 0;
        heads[i].id_len = id_len;
        heads[i].n_samples = ns;
        memcpy(&heads[i].digitisation, h + 16, 8);
        memcpy(&heads[i].offset, h + 24, 8);
        memcpy(&heads[i].range, h + 32, 8);
        heads[i].record_bytes = rec_off[i + 1] - rec_off[i];
        scaling[3 * i] = heads[i].digitisation;
        scaling[3 * i + 1] = heads[i].offset;
        scaling[3 * i + 2] = heads[i].range;
        raw_off[i + 1] = raw_off[i] + ns;
    }
    if (!fallback) {
        const int64_t total = raw_off[n];
        if ((rc = c->raw.reserve_samples(total, static_cast<size_t>(n)))) return rc;
        HIP_TRY(hipMemcpyAsync(c->raw.e_rawoff.p, raw_off.data(), 8 * static_cast<size_t>(n + 1), hipMemcpyHostToDevice, sp));
        sfa::SvbArgs sa{fa.payload, fa.payload_off, c->blow5.b_head.as<uint8_t>(), c->raw.e_rawoff.as<int64_t>(), c->raw.e_raw.as<int16_t>(), c->blow5.b_bad.as<int32_t>(),
                        signal_svb ? 1 : 0, n};
        hipLaunchKernelGGL(sfa::blow5_svb_kernel, dim3((n + 3) / 4), dim3(256), 0, sp, sa);
        KERNEL_TRY();
        int32_t *bad = reinterpret_cast<int32_t *>(hh + static_cast<size_t>(n) * sfa::kBlow5HeadBytes);
        HIP_TRY(hipMemcpyAsync(bad, c->blow5.b_bad.p, 4 * static_cast<size_t>(n), hipMemcpyDeviceToHost, sp));
        HIP_TRY(hipEventRecord(c->bev[1], sp));
        HIP_TRY(hipStreamSynchronize(sp));
        for (int32_t i = 0; i < n && !fallback; ++i)
            if (bad[i] != 0) {
                (void)fail(SFA_OK, "sfa_align_blow5: signal of record %d is shorter than its keys say: host reader takes the batch", i);
                fallback = true;
            }
        if (!fallback) {
            c->blow5.bev_pending = true;
            return align_raw_impl(c, nullptr, raw_off.data(), scaling.data(), n, prefix_size, query_size, rows, info, query_events);
        }
    }
    // host reader for the whole batch (own inflate / zlib, SSSE3 StreamVByte): malformed records are reported from there
    c->blow5.blow5_fallbacks++;
    std::vector<int16_t> raw;
    raw_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        sfa::Blow5Record rec;
        std::string err;
        if (!sfa::parse_blow5_record(records + rec_off[i], static_cast<size_t>(rec_off[i + 1] - rec_off[i]), record_zlib, signal_svb, &rec, &err))
            return fail(SFA_EINVAL, "sfa_align_blow5: record %d: %s", i, err.c_str());
        if (rec.read_id.size() > sizeof(heads[i].read_id) - 1) return fail(SFA_ERANGE, "sfa_align_blow5: record %d: read id of %zu bytes", i, rec.read_id.size());
        memcpy(heads[i].read_id, rec.read_id.c_str(), rec.read_id.size() + 1);
        heads[i].id_len = static_cast<int32_t>(rec.read_id.size());
        heads[i].n_samples = static_cast<int64_t>(rec.raw.size());
        heads[i].digitisation = rec.digitisation;
        heads[i].offset = rec.offset;
        heads[i].range = rec.range;
        heads[i].record_bytes = rec_off[i + 1] - rec_off[i];
        scaling[3 * i] = rec.digitisation;
        scaling[3 * i + 1] = rec.offset;
        scaling[3 * i + 2] = rec.range;
        raw.insert(raw.end(), rec.raw.begin(), rec.raw.end());
        raw_off[i + 1] = static_cast<int64_t>(raw.size());
    }
    if (raw.empty()) raw.push_back(0);
    return align_raw_impl(c, raw.data(), raw_off.data(), scaling.data(), n, prefix_size, query_size, rows, info, query_events);
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
    std::vector<int64_t> ev_off;  // as align_raw_impl: room for len + 2 records per read
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
