// stages.cpp -- what happens to one batch: load -> host stages -> GPU stage -> output (load_db, process_db, output_db of the
// reference, src/dtw_main.c:299-326), and the report at the end of the run.
#include <cstdio>
#include <cstring>

#include "../host/events.hpp"
#include "run.hpp"

namespace cli {
namespace {

constexpr int32_t kNoMap = INT32_MIN;

// row k of read i in print order: its primary (k = 0), then the candidates behind it, best first ...
const sfa_result_t &hit(const Slot &sl, int32_t i, int k) { return k == 0 ? sl.rows[i] : sl.sec[static_cast<size_t>(i) * 4 + (k - 1)]; }
// ... and the place of that row among the batch's event maps (Slot::map_rows)
size_t hit_index(const Slot &sl, int32_t i, int k) { return k == 0 ? static_cast<size_t>(i) : static_cast<size_t>(sl.n) + static_cast<size_t>(i) * 4 + (k - 1); }
bool mapped(const sfa_result_t &w) { return w.valid && w.rid >= 0; }
// a read with rows to print: mapped, and (host events) with a query window of its own
bool printable(const Run &run, const Slot &sl, int32_t i) { return mapped(sl.rows[i]) && (run.gpu_events || sl.reads[i].keep); }
const char *read_id(const Run &run, const Slot &sl, int32_t i) { return run.gpu_parse ? sl.heads[i].read_id : sl.reads[i].rec.read_id.c_str(); }

void reset(Read &r) { r.keep = false, r.ev.clear(), r.status = 0; }
bool parse_one(const Run &run, Read &r) {  // parse_single, src/sigfish.c:317-328
    std::string perr;
    const bool ok = r.view ? run.reader.parse(r.view, r.view_size, &r.rec, &perr) : run.reader.parse(r.mem, &r.rec, &perr);
    reset(r);
    return ok;
}
void events_one(const Run &run, Read &r, std::vector<float> &pa) {  // event_single, src/sigfish.c:330-378
    const int64_t ns = static_cast<int64_t>(r.rec.raw.size());
    pa.resize(ns);
    sfa::raw_to_picoamps(r.rec.raw.data(), ns, r.rec.digitisation, r.rec.offset, r.rec.range, pa.data());
    r.ev = sfa::detect_events(pa.data(), ns, (run.o.flag & F_RNA) != 0);
}
void normalise_one(const Run &run, Read &r, const std::vector<float> &pa) {  // normalise_single, src/sigfish.c:424-505
    if (!r.ev.empty())
        r.keep = sfa::select_and_normalise(r.ev, r.rec.raw.data(), static_cast<int64_t>(r.rec.raw.size()), pa.data(), run.o.prefix, run.o.query,
                                           run.o.flag, run.o.pore_flag, &r.qstart, &r.qend, &r.status);
}

// --gpu-parse: nothing to parse here, the records go to the device as they are
void stage_records(Run &run, Slot &sl) {
    const double b = realtime();
    const int32_t n = sl.n;
    sl.rec_off.resize(n + 1);
    sl.rec_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) sl.rec_off[i + 1] = sl.rec_off[i] + static_cast<int64_t>(sl.reads[i].view_size);
    sl.rec_bytes.grow(static_cast<size_t>(sl.rec_off[n]) + 64, &run.st.t_pin);
    uint8_t *dst = static_cast<uint8_t *>(sl.rec_bytes.data());
    run.pool.run(n, [&](int64_t i) { memcpy(dst + sl.rec_off[i], sl.reads[i].bytes(), static_cast<size_t>(sl.rec_off[i + 1] - sl.rec_off[i])); });
    run.st.add(run.st.t_parse, realtime() - b);
}

// one fan-out per batch, every read through all its host stages (work_per_single_read, src/sigfish.c:995-1001)
bool parse_fused(Run &run, Slot &sl) {
    std::vector<Read> &batch = sl.reads;
    const int32_t n = sl.n;
    std::atomic<int> bad(0);
    auto rest_of = [&](Read &r) {
        if (bad || run.gpu_events || r.rec.raw.empty()) return;
        std::vector<float> pa;
        events_one(run, r, pa);
        normalise_one(run, r, pa);
    };
    // reads go two at a time: their zlib streams are inflated side by side by one thread (blow5.hpp: parse_pair)
    run.pool.run((n + 1) / 2, [&](int64_t j) {
        const int64_t i0 = 2 * j, i1 = 2 * j + 1;
        if (i1 >= n) {
            if (!parse_one(run, batch[i0])) bad = 1;
        } else {
            Read &a0 = batch[i0], &a1 = batch[i1];
            const uint8_t *const mem[2] = {a0.bytes(), a1.bytes()};
            const size_t size[2] = {a0.view_size, a1.view_size};
            sfa::Blow5Record *const rec[2] = {&a0.rec, &a1.rec};
            std::string e0, e1;
            std::string *const perr[2] = {&e0, &e1};
            bool ok[2];
            run.reader.parse_pair(mem, size, rec, perr, ok);
            if (!ok[0] || !ok[1]) bad = 1;
            reset(a0);
            reset(a1);
            rest_of(a1);
        }
        rest_of(batch[i0]);
    });
    return !bad;
}

// --profile-cpu=yes: stage by stage, each under its timer
bool parse_sectional(Run &run, Slot &sl) {
    std::vector<Read> &batch = sl.reads;
    std::atomic<int> bad(0);
    double b = realtime();
    run.pool.run(sl.n, [&](int64_t i) { bad |= !parse_one(run, batch[i]); });
    run.st.add(run.st.t_parse, realtime() - b);
    if (run.gpu_events || bad) return !bad;
    b = realtime();
    run.pool.run(sl.n, [&](int64_t i) { if (!batch[i].rec.raw.empty()) events_one(run, batch[i], batch[i].pa); });
    run.st.add(run.st.t_events, realtime() - b);
    b = realtime();
    run.pool.run(sl.n, [&](int64_t i) {
        if (!batch[i].rec.raw.empty()) normalise_one(run, batch[i], batch[i].pa);
        std::vector<float>().swap(batch[i].pa);
    });
    run.st.add(run.st.t_norm, realtime() - b);
    return true;
}

// events on the device: pack the samples of the batch for one upload
void stage_samples(Run &run, Slot &sl) {
    const std::vector<Read> &batch = sl.reads;
    const int32_t n = sl.n;
    sl.raw_off.resize(n + 1);
    sl.scaling.resize(3 * static_cast<size_t>(n));
    sl.raw_off[0] = 0;
    for (int32_t i = 0; i < n; ++i) {
        sl.raw_off[i + 1] = sl.raw_off[i] + static_cast<int64_t>(batch[i].rec.raw.size());
        sl.scaling[3 * i] = batch[i].rec.digitisation;
        sl.scaling[3 * i + 1] = batch[i].rec.offset;
        sl.scaling[3 * i + 2] = batch[i].rec.range;
    }
    sl.raw.grow((static_cast<size_t>(sl.raw_off[n]) + 1) * sizeof(int16_t), &run.st.t_pin);
    int16_t *dst = static_cast<int16_t *>(sl.raw.data());
    run.pool.run(n, [&](int64_t i) { memcpy(dst + sl.raw_off[i], batch[i].rec.raw.data(), sizeof(int16_t) * batch[i].rec.raw.size()); });
}

// events on the host: the windows that normalise_one chose, as sfa_align_events takes them
void gather_windows(Run &run, Slot &sl) {
    std::lock_guard<std::mutex> lock(run.st.mu);
    for (int32_t i = 0; i < sl.n; ++i) {
        const Read &r = sl.reads[i];
        sl.evp[i] = r.keep ? r.ev.data() : nullptr;
        sl.nev[i] = r.keep ? static_cast<int64_t>(r.ev.size()) : 0;
        sl.qs[i] = r.qstart;
        sl.qe[i] = r.qend;
        run.st.count_status(r.status);
    }
}

// --sam --device-paths: one request for the event maps of every row of the batch that will be printed
void request_event_maps(const Run &run, Slot &sl, sfa_ctx_t *ctx) {
    const int32_t n = sl.n, nr = n * run.hits;
    sl.map_rows.assign(sl.rows.begin(), sl.rows.begin() + n);
    if (run.hits > 1) sl.map_rows.insert(sl.map_rows.end(), sl.sec.begin(), sl.sec.begin() + static_cast<size_t>(n) * 4);
    sl.map_read.resize(nr);
    sl.map_off.assign(static_cast<size_t>(nr) + 1, 0);
    for (int32_t k = 0; k < nr; ++k) {
        const sfa_result_t &w = sl.map_rows[k];
        sl.map_read[k] = k < n ? k : (k - n) / 4;
        const int64_t need = mapped(w) ? static_cast<int64_t>(w.pos_end) - w.pos_st + 1 : 0;
        sl.map_off[k + 1] = sl.map_off[k] + (need > 0 ? need : 0);
    }
    sl.map_pairs.resize(2 * static_cast<size_t>(sl.map_off[nr]) + 2);
    for (int32_t k = 0; k < nr; ++k) sl.map_pairs[2 * sl.map_off[k]] = kNoMap;
    if (sfa_event_maps(ctx, sl.map_rows.data(), sl.map_read.data(), nr, sl.map_off.data(), sl.map_pairs.data(), nullptr) != SFA_OK)
        die(std::string("event maps: ") + sfa_last_error());
}

// Formatted from the batch's event maps (device_paths); a row without one, and every row without --device-paths, has its
// warp path rebuilt here from its band (sam.hpp).  One read per task
void write_sam(Run &run, const Slot &sl) {
    const Opt &o = run.o;
    const Reference &ref = run.ref;
    std::vector<std::string> sam_rows(sl.n);
    run.pool.run(sl.n, [&](int64_t i) {
        if (!printable(run, sl, i)) return;
        const Read &r = sl.reads[i];
        // the event table and the window inside it: the read's own (host events) or the window alone (device events)
        const sfa_event_t *ev = run.gpu_events ? sl.qev.data() + static_cast<size_t>(i) * o.query : r.ev.data();
        const int64_t qs = run.gpu_events ? 0 : r.qstart, qe = run.gpu_events ? sl.info[i].qend - sl.info[i].qstart : r.qend;
        const char *rid = read_id(run, sl, i);
        for (int k = 0; k < run.hits; ++k) {
            const sfa_result_t &w = hit(sl, i, k);
            if (!mapped(w)) continue;
            const char *rname = ref.contigs[w.rid].name.c_str();
            std::string buf(1 << 16, '\0');
            const int32_t *map = nullptr;
            int32_t n_map = 0;
            if (run.device_paths) {
                const size_t mk = hit_index(sl, i, k);
                n_map = static_cast<int32_t>(sl.map_off[mk + 1] - sl.map_off[mk]);
                map = sl.map_pairs.data() + 2 * sl.map_off[mk];
                if (n_map <= 0 || map[0] == kNoMap) map = nullptr;
            }
            auto format = [&]() {
                return map ? sfa_sam_row_from_map(&buf[0], buf.size(), &w, rid, rname, ev, qs, qe, map, n_map, o.flag, k > 0)
                           : sfa_sam_row_ex(&buf[0], buf.size(), &w, rid, rname, ev, qs, qe, ref.events(w), ref.ref_len[w.rid], ref.ref_off[w.rid],
                                            o.flag, k > 0);
            };
            int len = format();
            if (len == SFA_ERANGE) {  // very long ss strings (full-reference alignments)
                buf.assign(1 << 22, '\0');
                len = format();
            }
            if (len > 0) sam_rows[i].append(buf.data(), len);
            else run.st.sam_unprintable.fetch_add(1, std::memory_order_relaxed);
        }
    });
    for (int32_t i = 0; i < sl.n; ++i) fwrite(sam_rows[i].data(), 1, sam_rows[i].size(), stdout);
}

// output_db + aln_to_str, src/sigfish.c:796-826,1051-1086; the candidates behind the primary print as tp:A:S, mapq 0
void write_paf(const Run &run, const Slot &sl) {
    std::string line(4096, '\0');
    for (int32_t i = 0; i < sl.n; ++i) {
        if (!printable(run, sl, i)) continue;
        const Read &r = sl.reads[i];
        uint64_t start_raw, end_raw, qsize;
        if (run.gpu_events) {
            start_raw = sl.info[i].start_raw_idx;
            end_raw = sl.info[i].end_raw_idx;
            qsize = static_cast<uint64_t>((sl.info[i].qend - 1) - sl.info[i].qstart);
        } else {
            const sfa_event_t &e0 = r.ev[r.qstart], &e1 = r.ev[r.qend - 1];
            start_raw = e0.start;
            end_raw = static_cast<uint64_t>(static_cast<float>(e1.start) + e1.length);  // u64 + float, as in C
            qsize = static_cast<uint64_t>((r.qend - 1) - r.qstart);
        }
        const uint64_t n_raw = run.gpu_parse ? static_cast<uint64_t>(sl.heads[i].n_samples) : r.rec.raw.size();
        const char *rid = read_id(run, sl, i);
        for (int k = 0; k < run.hits; ++k) {
            const sfa_result_t &w = hit(sl, i, k);
            if (!mapped(w)) continue;
            const int len = sfa_paf_row_ex(&line[0], line.size(), &w, rid, run.ref.contigs[w.rid].name.c_str(), start_raw, end_raw, qsize,
                                           n_raw, static_cast<uint64_t>(run.ref.seq_len[w.rid]), k > 0 ? 'S' : 'P');
            if (len < 0) die("PAF line too long");
            fwrite(line.data(), 1, len, stdout);
        }
    }
}

}  // namespace

// The device route decodes BLOW5 records; the lines of a SLOW5 ASCII file are parsed by the host threads.  Measured on one GPU
// with 16 host threads (profiles/r02_logs/e2e_compressed_streams_x_batch.log): the two routes are level, 0.49-0.52 M reads/s
// from a compressed file -- 16 cores inflate 0.75 M records/s, the device 1.0 M/s but in competition with the alignment kernels
// for the same LDS -- and the host route is the better one at the default -K 4096.  What the device route buys is independence
// from the host: a node's cores do not grow with its GPUs, so it is the default from three devices on.
bool choose_gpu_parse(const Opt &o, const sfa::Blow5Reader &reader) {
    if (reader.ascii() && o.gpu_parse == 1) die("--gpu-parse decodes BLOW5 records: a SLOW5 ASCII file is parsed on the host threads");
    // zstd records (record_press 2): the host threads unless --gpu-parse asks for the device (DESIGN.md section 6 has the measurement)
    const bool by_default = reader.record_press() == 2 ? false : o.devices.size() > 2;
    return !o.host_events && !reader.ascii() && (o.gpu_parse < 0 ? by_default : o.gpu_parse == 1);
}

bool load_batch(Run &run, Slot &sl) {
    const Opt &o = run.o;
    std::vector<Read> &batch = sl.reads;
    const double a = realtime();
    sl.n = 0;
    sl.bytes = 0;
    bool more = true;
    if (run.loader) {
        const Frames &f = run.loader->next();
        if (f.failed) die(run.reader.error());
        sl.n = f.n;
        sl.bytes = f.bytes;
        more = f.more;
        for (int32_t i = 0; i < f.n; ++i) {
            batch[i].view = f.view[i];
            batch[i].view_size = f.size[i];
        }
    }
    while (!run.loader && sl.n < o.batch_size && sl.bytes < o.batch_bytes) {
        Read &r = batch[sl.n];
        int rc = run.reader.next_view(&r.view, &r.view_size);
        if (rc == -2) {  // not mappable: copy the record
            r.view = nullptr;
            rc = run.reader.next_mem(&r.mem);
            r.view_size = r.mem.size();
        }
        if (rc < 0) die(run.reader.error());
        if (rc == 0) {
            more = false;
            break;
        }
        sl.bytes += static_cast<int64_t>(r.view_size);
        ++sl.n;
    }
    run.st.t_load += realtime() - a;
    if (o.verbosity >= 4)
        fprintf(stderr, "[dtw_main::%.3f*%.2f] %d Entries (%.1fM bytes) loaded\n", realtime() - run.t0, cputime() / (realtime() - run.t0), sl.n, sl.bytes / 1e6);
    return more;
}

void host_stages(Run &run, Slot &sl) {
    const double a = realtime();
    if (run.gpu_parse) {
        stage_records(run, sl);
    } else {
        if (!(run.prf ? parse_sectional(run, sl) : parse_fused(run, sl))) die("error parsing a BLOW5 record");
        if (run.gpu_events) stage_samples(run, sl);
        else gather_windows(run, sl);
    }
    run.st.t_proc += realtime() - a;
}

void align_stage(Run &run, Slot &sl, sfa_ctx_t *ctx) {
    const Opt &o = run.o;
    const int32_t n = sl.n;
    sfa_result_t *rows = sl.rows.data();
    const double a = realtime();
    if (run.gpu_events) {
        sl.info.resize(n);
        if (run.sam) sl.qev.resize(static_cast<size_t>(n) * o.query);
    }
    sfa_profile_t pr{};
    if (n > 0) {  // (an empty batch starts nothing on the device)
        sfa_event_t *qev = run.sam ? sl.qev.data() : nullptr;
        int rc;
        if (run.gpu_parse) {
            sl.heads.resize(n);
            rc = sfa_align_blow5(ctx, static_cast<const uint8_t *>(sl.rec_bytes.data()), sl.rec_off.data(), n, run.reader.record_press(),
                                 run.reader.signal_svb(), o.prefix, o.query, rows, sl.info.data(), sl.heads.data(), qev);
        } else if (run.gpu_events) {
            rc = sfa_align_raw_ex(ctx, static_cast<const int16_t *>(sl.raw.data()), sl.raw_off.data(), sl.scaling.data(), n, o.prefix, o.query, rows,
                                  sl.info.data(), qev);
        } else {
            rc = sfa_align_events(ctx, sl.evp.data(), sl.nev.data(), sl.qs.data(), sl.qe.data(), n, rows);
        }
        if (rc != SFA_OK) die(std::string("alignment failed: ") + sfa_last_error());
        if (run.hits > 1) {
            sl.sec.resize(static_cast<size_t>(n) * 4);
            if (sfa_secondary_rows(ctx, sl.sec.data(), n) != SFA_OK) die(std::string("secondary mappings: ") + sfa_last_error());
        }
        if (run.device_paths) request_event_maps(run, sl, ctx);
        if (run.prf && sfa_get_profile(ctx, &pr) != SFA_OK) die(std::string("sfa_get_profile failed: ") + sfa_last_error());
    }
    Stats &st = run.st;
    std::lock_guard<std::mutex> lock(st.mu);
    st.t_dtw += realtime() - a;
    if (run.prf) {
        if (run.gpu_events) {  // events and normalisation ran on the device, inside the same call
            st.t_parse += pr.decode_ms * 1e-3;  // ... and so did parse_single's work, when the records went up as they are
            st.t_events += pr.events_ms * 1e-3;
            st.t_norm += pr.normalise_ms * 1e-3;
            st.t_dtw_stage += pr.total_ms * 1e-3;
        } else {
            st.t_dtw_stage += realtime() - a;  // the reference's timer around align_db (src/sigfish.c:1037-1040)
        }
    }
    for (int32_t i = 0; i < n && run.gpu_events; ++i) st.count_status(sl.info[i].status);
    if (o.verbosity >= 4)
        fprintf(stderr, "[dtw_main::%.3f*%.2f] %d Entries (%.1fM bytes) processed\n", realtime() - run.t0, cputime() / (realtime() - run.t0), n, sl.bytes / 1e6);
}

void output_stage(Run &run, Slot &sl) {
    const double a = realtime();
    if (run.sam) write_sam(run, sl);
    else write_paf(run, sl);
    fflush(stdout);
    run.st.add(run.st.t_out, realtime() - a);
}

void Stats::report(const Opt &o, bool prf) const {
    if (sam_unprintable.load() > 0 && o.verbosity >= 1)
        fprintf(stderr, "[sigfish-amd] WARNING: %ld mapped row(s) have no SAM record: the ss string cannot express their warp path (RNA: last reference column without a query event)\n",
                (long)sam_unprintable.load());
    if (o.verbosity >= 3 && prf) {  // the reference's lines, src/dtw_main.c:331-343
        fprintf(stderr, "[dtw_main] total entries: %ld\tprefix fail: %ld\tignored: %ld\ttoo short: %ld", (long)total, (long)prefix_fail, (long)ignored, (long)too_short);
        fprintf(stderr, "\n[dtw_main] total bytes: %.1f M", sum_bytes / 1e6);
        fprintf(stderr, "\n[dtw_main] Data loading time: %.3f sec", t_load);
        fprintf(stderr, "\n[dtw_main] Data processing time: %.3f sec", t_proc + t_dtw);
        fprintf(stderr, "\n[dtw_main]     - Parse time: %.3f sec", t_parse);
        fprintf(stderr, "\n[dtw_main]     - Events time: %.3f sec", t_events);
        fprintf(stderr, "\n[dtw_main]     - Normalise time: %.3f sec", t_norm);
        fprintf(stderr, "\n[dtw_main]     - DTW time: %.3f sec", t_dtw_stage);
        fprintf(stderr, "\n[dtw_main] Data output time: %.3f sec\n", t_out);
    } else if (o.verbosity >= 3) {
        fprintf(stderr, "[dtw_main] total entries: %ld\tprefix fail: %ld\tignored: %ld\ttoo short: %ld\n", (long)total, (long)prefix_fail, (long)ignored, (long)too_short);
        fprintf(stderr, "[dtw_main] total bytes: %.1f M\n[dtw_main] Data loading time: %.3f sec\n", sum_bytes / 1e6, t_load);
        fprintf(stderr, "[dtw_main] Data processing time: %.3f sec (host stages) + %.3f sec (DTW stage, overlapped with the next batch)\n",
                t_proc, t_dtw);
        fprintf(stderr, "[dtw_main] Data output time: %.3f sec\n", t_out);
        if (o.verbosity >= 4)
            fprintf(stderr, "[dtw_main] main thread waited %.3f sec for a free device context and %.3f sec for the printer; page-locked staging (re)allocated in %.3f sec (inside the host stages)\n",
                    t_wait_gpu, t_wait_out, t_pin);
    }
}

}  // namespace cli
