// run.hpp -- the state of one `sigfish-amd dtw` run and the stages a batch goes through (stages.cpp):
// load_batch -> host_stages on the main thread, align_stage on the GPU-stage helper of the batch's context,
// output_stage on the printer.
#pragma once
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/sigfish_amd.h"
#include "../host/blow5.hpp"
#include "../host/refio.hpp"
#include "cli.hpp"
#include "frame_loader.hpp"
#include "worker_pool.hpp"

namespace cli {

struct Read {
    std::vector<uint8_t> mem;          // record bytes when the file cannot be mapped
    const uint8_t *view = nullptr;     // record bytes inside the mapped file otherwise
    size_t view_size = 0;
    sfa::Blow5Record rec;
    std::vector<sfa_event_t> ev;
    std::vector<float> pa;             // --profile-cpu=yes: picoamps kept between the events and the normalise stage
    int64_t qstart = 0, qend = 0;
    bool keep = false;
    int status = 0;
    const uint8_t *bytes() const { return view ? view : mem.data(); }
};

// Page-locked staging (sfa_pinned_alloc), grown on demand by the main thread and released with its slot.  Move-only: declaring
// the move constructor leaves no copy operations.
class PinnedBuffer {
  public:
    explicit PinnedBuffer(const char *what) : what_(what) {}
    PinnedBuffer(PinnedBuffer &&b) noexcept : p_(b.p_), cap_(b.cap_), what_(b.what_) { b.p_ = nullptr, b.cap_ = 0; }
    ~PinnedBuffer() { sfa_pinned_free(p_); }
    // room for `need` bytes (a quarter more when it has to be allocated again; contents are not kept); the time goes to *t_pin
    void grow(size_t need, double *t_pin) {
        if (need <= cap_) return;
        const double a = realtime();
        sfa_pinned_free(p_);
        cap_ = need + need / 4;
        p_ = sfa_pinned_alloc(cap_);
        *t_pin += realtime() - a;
        if (!p_) die(std::string("cannot allocate the ") + what_ + " staging buffer: " + sfa_last_error());
    }
    void *data() const { return p_; }

  private:
    void *p_ = nullptr;
    size_t cap_ = 0;
    const char *what_;
};

// One batch on its way through the pipeline.
struct Slot {
    std::vector<Read> reads;
    std::vector<const sfa_event_t *> evp;
    std::vector<int64_t> nev, qs, qe;
    std::vector<sfa_result_t> rows;
    std::vector<sfa_result_t> sec;  // --secondary yes: [n][4] rows behind each primary, best first
    // --sam --device-paths: the event maps of the batch from the device.  Row i is the primary of read i, row n + 4 i + k
    // its k-th secondary (hit_index); map_off in pairs; a map the library left unwritten keeps kNoMap in its first word
    std::vector<sfa_result_t> map_rows;
    std::vector<int32_t> map_read, map_pairs;
    std::vector<int64_t> map_off;
    // device-side event detection: concatenated raw samples + scaling instead of event tables
    PinnedBuffer raw{"sample"};
    std::vector<int64_t> raw_off;
    std::vector<double> scaling;
    std::vector<sfa_query_info_t> info;
    std::vector<sfa_event_t> qev;  // [n][query] event tables of the query windows (SAM with device-side events)
    // device-side record decoding: the records' bytes as they are in the file, back to back
    PinnedBuffer rec_bytes{"record"};
    std::vector<int64_t> rec_off;
    std::vector<sfa_read_head_t> heads;
    int32_t n = 0;
    int64_t bytes = 0;

    explicit Slot(int32_t batch_size) : reads(batch_size), evp(batch_size), nev(batch_size), qs(batch_size), qe(batch_size), rows(batch_size) {}
};

// Timers and counters of the run.  Every field names the thread that writes it; whatever a helper thread writes, and whatever
// the main thread writes while helpers may be running, is written under `mu`.  report() runs after the last helper is joined.
struct Stats {
    std::mutex mu;
    // main thread only
    double t_load = 0, t_proc = 0;
    double t_wait_gpu = 0, t_wait_out = 0;  // waiting for a context / for the printer
    double t_pin = 0;                       // page-locked staging (re)allocation, both buffers of every slot (PinnedBuffer::grow)
    int64_t total = 0, sum_bytes = 0;
    // GPU-stage helpers, under mu (two GPU stages may finish together)
    double t_dtw = 0, t_dtw_stage = 0;
    // main thread (host stages of the host routes; record staging) and GPU-stage helpers (device routes), under mu
    double t_parse = 0, t_events = 0, t_norm = 0;
    int64_t prefix_fail = 0, ignored = 0, too_short = 0;
    // printer helper, and the main thread for the last batches once the printer is joined; under mu
    double t_out = 0;
    // worker pool, inside the printer's fan-out.  Mapped rows without a SAM record: the writer refuses a map it cannot express (RNA
    // --dtw-std: a warp path that enters the last reference column without advancing in the query leaves it blank, where
    // r2qevent_map_to_ss asserts, src/sigfish.c:668-669)
    std::atomic<int64_t> sam_unprintable{0};

    void add(double &timer, double seconds) {
        std::lock_guard<std::mutex> lock(mu);
        timer += seconds;
    }
    void count_status(int status) {  // of one read's query window; the caller holds mu
        prefix_fail += (status & 4) != 0;
        ignored += (status & 2) != 0;
        too_short += (status & 1) != 0;
    }
    void report(const Opt &o, bool prf) const;  // the end-of-run lines on stderr (src/dtw_main.c:331-343)
};

// The contigs and their event arrays, and the view of them that sfa_init uploads.
struct Reference {
    std::vector<sfa::FastaRecord> contigs;
    std::vector<std::vector<float>> fwd, rev;  // rev stays empty for RNA
    std::vector<int32_t> ref_len, ref_off, seq_len;
    std::vector<const float *> fp, rp;
    sfa_ref_t view{};  // points into the vectors above

    // reads o.model_file and o.fasta; flag and query of `o` shape the events (after detect_chemistry)
    explicit Reference(const Opt &o);
    Reference(const Reference &) = delete;
    const float *events(const sfa_result_t &w) const { return w.strand == '+' ? fwd[w.rid].data() : rev[w.rid].data(); }
};
// RNA and pore from the file's header where the options left them open; runs before the reference is built
void detect_chemistry(const sfa::Blow5Reader &reader, Opt *o);

// What a stage needs besides its batch.  Everything but `st` is fixed once the pipeline starts.
struct Run {
    const Opt &o;
    const Reference &ref;
    sfa::Blow5Reader &reader;
    WorkerPool &pool;
    FrameLoader *loader;  // mapped files; anything else is read record by record
    const double t0;
    // events on the GPU (the RNA automatic query start, -p -1, included) unless --host-events; for SAM the event tables of the
    // query windows come back from the device with the rows
    // (gpu_parse: the records go to the device as they are in the file, sfa_align_blow5, choose_gpu_parse; device_paths: --sam with --device-paths)
    const bool gpu_events, gpu_parse, sam, device_paths;
    // --profile-cpu=yes (src/dtw_main.c:213-214, src/sigfish.c:1021-1040): the stages of a batch run one after the other,
    // each under its own timer, and the batches are not overlapped.  Host stages are wall time of their fan-out over -t
    // threads, as in the reference; stages that run on the device are the device's own time (HIP events, sfa_get_profile).
    const bool prf;
    const int hits;  // rows printed per read at the most: the primary, then (--secondary yes) four candidates behind it
    Stats st;
};
bool choose_gpu_parse(const Opt &o, const sfa::Blow5Reader &reader);

bool load_batch(Run &run, Slot &sl);  // false: the file (or this process's part of it) ends with this batch
void host_stages(Run &run, Slot &sl);
void align_stage(Run &run, Slot &sl, sfa_ctx_t *ctx);
void output_stage(Run &run, Slot &sl);

}  // namespace cli
