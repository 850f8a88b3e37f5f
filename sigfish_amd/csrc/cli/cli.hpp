// cli.hpp -- what every unit of the `sigfish-amd dtw` command line shares: the options, the clocks and how errors travel.
#pragma once
#include <sys/resource.h>
#include <sys/time.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace cli {

// option bits beyond the ones the library reads: same values as src/sigfish.h:30-39
enum : uint32_t { F_RNA = 0x001, F_DTW = 0x002, F_INV = 0x004, F_SEC = 0x008, F_REF = 0x010, F_END = 0x020, F_PRF = 0x040, F_SAM = 0x100, F_R10 = 0x200 };

struct Opt {
    uint32_t flag = 0;
    int32_t batch_size = 4096;            // -K  (reference default 512; a GPU batch wants thousands of reads)
    int64_t batch_bytes = 200 * 1000 * 1000;  // -B  (reference default 20M)
    int32_t threads = 8;
    int32_t prefix = 50, query = 250;
    int32_t debug_break = -1;
    int verbosity = 4;
    std::vector<int> devices{0};  // --device 0,1,...: batches go to the devices in turn
    bool host_events = false;  // --host-events: event detection on host threads instead of the GPU
    int gpu_parse = -1;        // --gpu-parse / --host-parse: records decompressed and parsed on the GPU / on host threads (-1: by device count)
    int streams = 0;           // --streams: device contexts that take batches in turn (0 = 2)
    // read sharding over processes (one per GPU): what part of the file THIS process maps
    int ranks = 0;                       // --ranks G: start G processes on disjoint parts of the file, print their output in rank order (0: one per distinct device)
    int shard_r = 0, shard_n = 1;        // --shard r/G: the records starting in the r-th of G equal byte slices of the file
    int64_t range_a = 0, range_b = -1;   // --read-range A:B: records [A, B) by position in the file (B omitted: to the end)
    bool no_header = false;              // --no-header: no SAM header (every rank but the first of a sharded run)
    int64_t rank_buffer = 256 * 1000 * 1000;  // --rank-buffer: gathered output kept in memory per rank; what exceeds it goes to an unnamed temporary file
    int device_share = 1;                // ranks of a sharded run that were given the same device as this one (a one-GPU rehearsal of --ranks)
    const char *model_file = nullptr;
    const char *pore = nullptr;
    int pore_flag = 0;  // 0 r9, 1 r10, 2 rna004
    bool device_paths = false;  // --device-paths: SAM from the event maps of a whole batch, computed on the GPU (sfa_event_maps); --host-paths
                                // (the default until the device route has been measured): warp paths rebuilt read by read on the host threads
    bool secondary = false;  // --secondary yes: print the candidates behind each primary (sfa_secondary_rows)
    bool secondary_strips = false;  // --secondary-strips: ... also for reads beyond 2048 events (the option "secondary_strips"; lifts the refusal of -q > 2048)
    const char *fasta = nullptr, *blow5 = nullptr;  // the two positional arguments
};

inline double realtime() {
    timeval tv;
    gettimeofday(&tv, nullptr);
    return tv.tv_sec + tv.tv_usec * 1e-6;
}
inline double cputime() {
    rusage r;
    getrusage(RUSAGE_SELF, &r);
    return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}

// Errors travel as exceptions: die() may be called on a helper thread (the GPU stage or the output stage of a batch,
// both std::async) while the main thread, the worker pool and another GPU stage are still running.  exit() from there
// would run static destructors and the HIP runtime's teardown under live kernels and threads; instead the exception
// crosses the future, the stack unwinds (futures of std::async wait for their thread, the pool joins its workers) and
// dtw_main() prints the message and returns the failure status from the main thread.
struct Fatal : std::runtime_error {
    using std::runtime_error::runtime_error;
};
[[noreturn]] inline void die(const std::string &msg) { throw Fatal(msg); }

// `sigfish-amd realtime`: the options it shares with dtw (flag, prefix = skip, query, threads, devices, model, pore, verbosity,
// the two files) and its own
struct RealtimeOpt {
    Opt o;
    int32_t channels = 512;        // --channels: slots of the session, reads in flight
    int64_t chunk_samples = 1600;  // --chunk-samples: samples a channel sends per tick
    int32_t norm_events = -1;      // --norm-events: calibration window (-1: the value of -q, the batch normalisation)
    int32_t min_events = -1;       // --min-events: no early decision below this many query events (-1: the value of -q)
    int32_t min_mapq = 61;         // --min-mapq: early decision at this mapq (61: never, mapq ends at 60)
    bool pace = false;             // --pace yes: tick t does not start before t x chunk_samples / sampling_rate seconds
    std::vector<int32_t> recal_at; // --recalibrate: window lengths at which a slot is renormalised ("double" is expanded)
    bool recal_at_end = false;     // --recalibrate-at-end: a read that ends short is normalised over all its query events
                                   // (SFA_RECAL_AT_END), and q is the last of recal_at, so a full read over q
    bool resweep = false;          // --resweep: the session is created with SFA_SESSION_RESWEEP (lifts --rna's need for --invert)
    int32_t candidates = 0;        // --candidates: candidate lines (tp:A:S) behind every primary line, 1..4 (0: none)
    bool spread = false;           // --spread: one context over the whole --device list (sfa_init_devices), the session with SFA_SESSION_SPREAD
    std::string targets;           // --targets FILE.bed: the session's targets; the early decision is the class decision (replay.hpp)
    int32_t target_mode = -1;      // --enrich: 0, --deplete: 1 (exactly one of them with --targets)
    bool by_name = false;          // --by-name: the BED file's name column sets the session's target groups; lines gain tg / gm (replay.hpp)
    int64_t quota = 0;             // --quota N: accepted reads after which a named group is closed (needs --by-name --enrich; 0: off)
    int32_t group_cap = 0;         // --group-cap N: a named group's columns close where accepted reads cover them N times (needs --by-name --enrich; 0: off)
    int32_t depth_cap = 0;         // --depth-cap N: target positions covered N times by accepted reads close (needs --targets --enrich, no --by-name; 0: off)
    int32_t lead = -1;             // --lead N: reach targets (sfa_session_targets_reach), N bases in front of every target in the read's direction (needs --targets, no --by-name; -1: off)
    int32_t group_lead = -1;       // --group-lead N: reach groups (sfa_session_target_groups_reach), N bases in front of every named target carry its label; the mask gets the same lead (needs --by-name --enrich; -1: off)
    bool group_stranded = false;   // --group-stranded: column 6 of the BED file is the target's strand (needs --group-lead)
    bool stranded = false;         // --stranded: column 6 of the BED file is the target's strand ('+', '-', '.'; needs --lead)
    float margin = 0.0f;           // --margin X: cost per query event between the classes (required with --targets: no default)
    std::string truth;             // --truth FILE.paf: where every read came from; lines gain tt / tv (tn / gv), the trace verdict lines (needs --targets)
    std::string trace;             // --trace FILE: the schedule's trace lines (replay.hpp)
};

// options.cpp: the option table, help and every check that needs no file and no device (exits for -V and help)
Opt parse_options(int argc, char **argv);
RealtimeOpt parse_realtime_options(int argc, char **argv);
// ranks.cpp
int supervise_ranks(Opt &o, double t0);

}  // namespace cli
