// dtw_main.cpp -- `sigfish-amd dtw`: the reference's `sigfish dtw` command line (src/dtw_main.c:125-352) over the
// MI355X alignment stage.  Same positional arguments, options and PAF output; the batch loop keeps the reference's
// order (load -> process -> output, src/dtw_main.c:299-326) so reads come out in file order.
//
// Host stages run on a thread fan-out per batch (parse, events, normalise: src/sigfish.c:317-505); the DTW stage
// is one call into the C-ABI (sfa_align_events, the align_db hook).  There is no CPU DTW path in this binary.

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <memory>
#include <utility>

#include "run.hpp"

namespace cli {
namespace {

struct Contexts : std::vector<sfa_ctx_t *> {  // destroyed on every way out, after the helper threads that use them
    using std::vector<sfa_ctx_t *>::vector;
    ~Contexts() {
        for (sfa_ctx_t *c : *this) sfa_destroy(c);
    }
};

// SFA_OPTS="name=value,name=value": planner / launch options of the library (sfa_set_option) for experiments from the
// command line; rows do not depend on them (the library's test hooks are not options: refused here whatever the environment)
std::vector<std::pair<std::string, long long>> library_options_from_env() {
    std::vector<std::pair<std::string, long long>> out;
    const char *e = getenv("SFA_OPTS");
    const std::string all(e ? e : "");
    for (size_t p = 0; p < all.size();) {
        const size_t q = std::min(all.find(',', p), all.size());
        const std::string kv = all.substr(p, q - p);
        const size_t eq = kv.find('=');
        if (eq == std::string::npos || eq == 0) die("SFA_OPTS takes name=value[,name=value...]");
        if (kv.compare(0, 6, "debug_") == 0) die("SFA_OPTS: '" + kv.substr(0, eq) + "' is a test hook of the library, not an option");
        out.emplace_back(kv.substr(0, eq), atoll(kv.c_str() + eq + 1));
        p = q + 1;
    }
    return out;
}

// Two contexts (streams + scratch) on the same device: consecutive batches alternate between them, so the uploads
// and the event detection of batch i+1 overlap the DTW of batch i
// (--streams: more than two were measured to add nothing, the stages of one batch already serialise on syncs)
// Several devices (--device 0,1,...): reads shard by batch, every device holds its own copy of the reference
// arrays (uploaded by sfa_init: a single process needs no collective), rows come back in batch order.
void open_contexts(Contexts &ctxs, const Opt &o, const Reference &ref) {
    const int n_ctx = static_cast<int>(ctxs.size()), n_dev = static_cast<int>(o.devices.size());
    const auto from_env = library_options_from_env();
    for (int j = 0; j < n_ctx; ++j) {
        if (sfa_init(&ctxs[j], &ref.view, o.flag, o.devices[j % n_dev]) != SFA_OK) die(std::string("accelerator init failed: ") + sfa_last_error());
        // the small-batch shapes pay off while ONE batch leaves the chip idle; with s batches in flight per device the
        // threshold (waves per SIMD of a single batch) shrinks accordingly
        const int per_dev = n_ctx / n_dev * o.device_share;  // batches in flight on this device, all processes
        if (sfa_set_option(ctxs[j], "widen_below", std::max(1, 5 / per_dev)) != SFA_OK) die(sfa_last_error());
        // the pore reaches the device route's automatic query start (-p -1), as it reaches select_and_normalise on the host route
        if (sfa_set_pore(ctxs[j], o.pore_flag) != SFA_OK) die(sfa_last_error());
        if (o.secondary && sfa_set_option(ctxs[j], "secondary", 4) != SFA_OK) die(sfa_last_error());
        if (o.secondary_strips && sfa_set_option(ctxs[j], "secondary_strips", 1) != SFA_OK) die(sfa_last_error());
        // --sam --device-paths: queries beyond 2048 events (-q) keep their event maps on the device too, in row strips
        if (o.device_paths && sfa_set_option(ctxs[j], "map_strips", 1) != SFA_OK) die(sfa_last_error());
        for (const auto &nv : from_env)
            if (sfa_set_option(ctxs[j], nv.first.c_str(), nv.second) != SFA_OK) die(std::string("SFA_OPTS: ") + sfa_last_error());
    }
}

// This process's part of the file.  Finding it means walking the size prefixes of every record in front of it (0.36 us each: 0.3 s
// for the second half of a 1.6 M-read file), which needs nothing but the mapping: a helper thread does it while the main thread
// reads the model, builds the reference events and brings up the device contexts (0.3-0.4 s).  Joined in front of the batch loop.
bool select_part(sfa::Blow5Reader &reader, const Opt &o) {
    if (o.shard_n > 1 && !reader.select_shard(static_cast<uint32_t>(o.shard_r), static_cast<uint32_t>(o.shard_n))) return false;
    if ((o.range_a > 0 || o.range_b >= 0) &&
        !reader.select_records(static_cast<uint64_t>(o.range_a), o.range_b < 0 ? UINT64_MAX : static_cast<uint64_t>(o.range_b - o.range_a)))
        return false;
    reader.start_prefault();  // a helper thread takes the page faults of the mapped file ahead of the batch loop (blow5.hpp)
    return true;
}

struct Ended { int rc, verbosity; };  // verbosity of the run whose state has just been released (0: none was, the ranks were supervised)

Ended dtw_run(int argc, char **argv, double t0) {
    Opt o = parse_options(argc, argv);
    if (o.ranks > 1) {
        const int rc = supervise_ranks(o, t0);
        if (rc >= 0) return {rc, 0};
    }

    // ---- init_core(), src/sigfish.c:81-207 ----
    double ti = realtime();
    auto lap = [&ti] {  // seconds since the last call
        const double was = ti;
        return (ti = realtime()) - was;
    };
    sfa::Blow5Reader reader;
    if (!reader.open(o.blow5)) die(reader.error());
    std::future<bool> selected = std::async(std::launch::async, [&reader, &o] { return select_part(reader, o); });
    const double t_reader = lap();
    detect_chemistry(reader, &o);
    const Reference ref(o);
    const double t_reference = lap();
    const int n_ctx = (o.streams > 0 ? o.streams : 2) * static_cast<int>(o.devices.size());
    Contexts ctxs(n_ctx, nullptr);
    open_contexts(ctxs, o, ref);
    const double t_contexts = lap();
    if (!selected.get()) die(reader.error());
    const double t_select = lap();  // what of the walk the initialisation did not hide
    if (o.verbosity >= 4 && (o.shard_n > 1 || o.range_a > 0)) fprintf(stderr, "[dtw_main::%.3f] waited %.3f s more for this process's part of the file\n", realtime() - t0, t_select);
    if (o.verbosity >= 4)
        fprintf(stderr, "[dtw_main::%.3f] initialised: input %.3f s, model + reference events %.3f s, %d device context(s) %.3f s\n", realtime() - t0,
                t_reader, t_reference, n_ctx, t_contexts);

    const bool sam = (o.flag & F_SAM) != 0;
    if (sam && !o.no_header) {  // sam_hdr_wr(), src/dtw_main.c:118-123 (LN is the k-mer count, as the reference prints it)
        for (size_t i = 0; i < ref.contigs.size(); ++i) fprintf(stdout, "@SQ\tSN:%s\tLN:%ld\n", ref.contigs[i].name.c_str(), static_cast<long>(ref.ref_len[i]));
        fprintf(stdout, "@PG\tID:sigfish\tPN:sigfish\tVN:0.2.0\n");
    }

    // ---- batch loop, src/dtw_main.c:299-326, as a pipeline over n_ctx + 2 slots: while the GPU stages of batches i and i-1
    // (one per context) and the output of batch i-2 run on helper threads, the main thread loads and pre-processes
    // batch i+1.  Batches are printed strictly in order, so the output is the same as the serial loop's. ----
    // Order of the declarations = reverse order of release on every way out: the loader and the helper threads first (futures of
    // std::async wait for their thread), then the slots with their page-locked staging, the host threads, and the contexts last.
    WorkerPool pool(o.threads);  // -t host threads, alive for the whole run
    const bool gpu_parse = choose_gpu_parse(o, reader);
    const int n_slots = n_ctx + 2;  // one being filled, one per GPU stage in flight, one being printed
    std::vector<Slot> slots;
    slots.reserve(n_slots);
    for (int s = 0; s < n_slots; ++s) slots.emplace_back(o.batch_size);
    std::unique_ptr<FrameLoader> loader;  // (mapped files; anything else is read record by record)
    if (reader.mapped()) loader.reset(new FrameLoader(reader, o.batch_size, o.batch_bytes));
    Run run{o, ref, reader, pool, loader.get(), t0, !o.host_events, gpu_parse, sam, sam && o.device_paths, (o.flag & F_PRF) != 0, o.secondary ? 5 : 1, {}};
    Stats &st = run.st;
    std::vector<std::future<void>> gpu_pending(n_ctx);  // GPU stage per context
    std::future<void> out_pending;                      // output stage
    int64_t bi = 0;  // batch index; batch bi lives in slot bi % n_slots and runs on context bi % n_ctx
    for (bool more = true; more;) {
        Slot *sl = &slots[bi % n_slots];
        more = load_batch(run, *sl);
        host_stages(run, *sl);
        lap();
        if (gpu_pending[bi % n_ctx].valid()) gpu_pending[bi % n_ctx].get();  // batch bi-n_ctx has its rows, its context is free
        st.t_wait_gpu += lap();
        if (out_pending.valid()) out_pending.get();  // batch bi-n_ctx-1 is printed (its slot is filled next)
        st.t_wait_out += lap();
        if (bi >= n_ctx) {
            Slot *done = &slots[(bi - n_ctx) % n_slots];
            out_pending = std::async(std::launch::async, [&run, done] { output_stage(run, *done); });
        }
        sfa_ctx_t *c = ctxs[bi % n_ctx];
        gpu_pending[bi % n_ctx] = std::async(std::launch::async, [&run, sl, c] { align_stage(run, *sl, c); });
        if (run.prf) gpu_pending[bi % n_ctx].get();  // sectional mode: nothing of the next batch starts before this one is through
        st.total += sl->n;
        st.sum_bytes += sl->bytes;
        if (o.debug_break == bi++) break;
    }
    if (out_pending.valid()) out_pending.get();
    for (int64_t b = std::max<int64_t>(bi - n_ctx, 0); b < bi; ++b) {  // the last batches, in order
        if (gpu_pending[b % n_ctx].valid()) gpu_pending[b % n_ctx].get();
        output_stage(run, slots[b % n_slots]);
    }
    st.report(o, run.prf);
    if (o.verbosity >= 4) fprintf(stderr, "[dtw_main::%.3f] all output written; releasing the device\n", realtime() - t0);
    return {0, o.verbosity};
}

}  // namespace
}  // namespace cli

int dtw_main(int argc, char **argv) {
    using namespace cli;
    const double t0 = realtime();
    try {
        const Ended end = dtw_run(argc, argv, t0);
        // (--verbose 4: where a short run's tail goes -- contexts, page-locked buffers, the mapped file and the slots have been
        // released by now; what follows is the runtime's own exit.  Measured on a compressed 400 000-read file: release 0.06-0.10 s,
        // exit 0.12 s; leaving everything to the kernel with _exit() right after the last line takes the same 0.18-0.2 s, and
        // bringing the contexts up beside the first batches (parsing ahead into spare slots) gains what the spare slots then cost
        // at exit: profiles/r03_logs/rejected_cli_async_init_run_ahead_and_fast_exit.log)
        if (end.verbosity >= 4) fprintf(stderr, "[dtw_main::%.3f] device contexts, staging buffers and the file mapping released\n", realtime() - t0);
        return end.rc;
    } catch (const Fatal &e) {  // every helper thread has been joined by the unwinding (see Fatal)
        fflush(stdout);
        fprintf(stderr, "[sigfish-amd] ERROR: %s\n", e.what());
        return EXIT_FAILURE;
    }
}

int eval_main(int argc, char **argv);      // eval_main.cpp
int realtime_main(int argc, char **argv);  // realtime_main.cpp

int main(int argc, char **argv) {
    if (argc >= 2 && (!strcmp(argv[1], "--version") || !strcmp(argv[1], "-V"))) {
        fprintf(stdout, "sigfish-amd %s\n", sfa_version());
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "dtw")) return dtw_main(argc - 1, argv + 1);
    if (argc >= 2 && !strcmp(argv[1], "eval")) return eval_main(argc - 1, argv + 1);
    if (argc >= 2 && !strcmp(argv[1], "realtime")) return realtime_main(argc - 1, argv + 1);
    fprintf(argc >= 2 && (!strcmp(argv[1], "--help") || !strcmp(argv[1], "-h")) ? stdout : stderr,
            "Usage: sigfish-amd <command> [options]\n\ncommand:\n         dtw           map raw signal reads to a reference with subsequence DTW on an MI355X\n         eval          compare a test PAF with a truth PAF (mapping accuracy)\n         realtime      replay a BLOW5 file through a raw-signal session, channel by channel, a PAF line per decided read\n\n");
    return (argc >= 2 && (!strcmp(argv[1], "--help") || !strcmp(argv[1], "-h"))) ? 0 : 1;
}
