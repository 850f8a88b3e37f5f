// events.hpp -- host pre-DP stages of the `dtw` path: raw signal -> pA -> events ->
// query window -> z-normalised query.  Arithmetic follows the reference operation by operation (types and
// evaluation order included) so that the event means handed to the GPU are bit-identical.
#pragma once
#include <cstdint>
#include <vector>

#include "../../../include/sigfish_amd.h"

namespace sfa {

// event_single(), src/sigfish.c:330-350: pA = ((float)raw + offset) * (range / digitisation), all in fp32
void raw_to_picoamps(const int16_t *raw, int64_t n, double digitisation, double offset, double range, float *out);

// getevents(), src/events.c:557-577 -> detect_events() 510-554 (scrappie's t-statistic peak picker)
std::vector<sfa_event_t> detect_events(const float *pa, int64_t n, bool rna);

// RNA "-p -1": detect_query_start(), src/sigfish.c:380-422 (adaptor + poly-A segmenters, src/jnn.c)
// returns the first event index after the poly-A tail or -1
int64_t detect_query_start(const int16_t *raw, int64_t n, const float *pa, const std::vector<sfa_event_t> &ev, int pore);

// what detect_query_start() computes before it looks at events: the sample index polya.y + ad.y behind the poly-A tail that
// follows the adaptor, or -1 when either segmenter fails (n <= 2000 among the causes).  Applied to a PREFIX of a read it is the
// target of a raw session's automatic query start (sfa_session_raw_auto_start)
int64_t auto_start_target(const int16_t *raw, int64_t n, const float *pa, int pore);

// normalise_single(), src/sigfish.c:424-505: choose [qstart,qend), z-normalise the event means in place.
// Returns false when the read is dropped (et.n = 0 in the reference).  *status: 0 ok, 1 too short (kept),
// 2 ignored, |4 when the automatic prefix detection failed (fallback 50).
bool select_and_normalise(std::vector<sfa_event_t> &ev, const int16_t *raw, int64_t nraw, const float *pa, int32_t prefix_size,
                          int32_t query_size, uint32_t flag, int pore, int64_t *qstart, int64_t *qend, int *status);

// The same detector fed a read in chunks.  After a push the peak picker has walked every position j <= N - w_long (N samples
// seen, N >= 2 w_long): there both t-statistics are what the whole read will give, so every event whose closing peak has fired
// equals the event detect_events() reports over the complete read, all four fields bit for bit; finish() walks the remaining
// positions as the batch code does (zeros past n - w) and closes the last event at the end of the signal.  The state is a
// constant number of words: a ring of the last 2 w_long + 1 prefix sums, the two detectors, the sums at each detector's candidate
// peak and at the open event's start.
class EventStream {
   public:
    EventStream(double digitisation, double offset, double range, bool rna);
    // the events the samples raw[0..n) make final are written to out (at most cap); returns their number.  When that exceeds cap
    // nothing is consumed: the stream is as before the call
    int64_t push(const int16_t *raw, int64_t n, sfa_event_t *out, int64_t cap);
    int64_t finish(sfa_event_t *out, int64_t cap);  // end of the read: the rest, by the same rule; -1 once it has delivered
    int64_t samples() const { return st_.n; }

    static constexpr int kRing = 29;  // 2 * 14 + 1: the RNA long window
    struct Det {
        int64_t masked_to = 0, peak_pos = -1;
        float peak_value = 3.402823466e+38f;  // FLT_MAX
        bool valid_peak = false;
        double ps = 0.0, pq = 0.0;  // sum, sumsq at peak_pos
    };
    struct State {
        int64_t n = 0, next = 0;  // samples seen, first position the picker has not walked
        double acc = 0.0, acc2 = 0.0;
        double ring_s[kRing], ring_q[kRing];  // sum[i], sumsq[i] at i % ring
        Det det[2];                           // short, long
        int64_t ev_start = 0;                 // the open event
        double es = 0.0, eq = 0.0;
        bool any_cut = false, finished = false;
    };

   private:
    int64_t walk(State &s, int64_t upto, int64_t n_final, sfa_event_t *out, int64_t cap, int64_t emitted) const;
    State st_;
    int w1_, w2_, ring_;
    float thr1_, thr2_, peak_height_, offf_, unit_;
};

}  // namespace sfa
