// pre_rules.hpp -- the host rules of the stages in front of the DP (pure C++, no HIP; tests/c/pre_rules.cpp runs them without a
// GPU), each stated ONCE for the batch entry points (sfa_pre.hip), the sessions (sfa_session.hip) and the host twin
// (host/events.cpp): the detector's parameters, the adaptor segmenter's per pore, the fp32 scaling of event_single(), the room a
// read's events need, and the query window of normalise_single() with the status it reports.  The independent pin of the window
// rule is oracle/sdtw_oracle.c (orc_query_window).
#pragma once
#include <stdint.h>

namespace sfa {

// scrappie's event detector, src/events.c:47-58: short and long window, their thresholds, the peak height
struct DetectorParams {
    int32_t w1, w2;
    float thr1, thr2, peak_height;
};
inline DetectorParams detector_params(bool rna) { return rna ? DetectorParams{7, 14, 2.5f, 9.0f, 1.0f} : DetectorParams{3, 6, 1.4f, 9.0f, 0.2f}; }

// jnnv2()'s shortest adaptor and the scale of its threshold: JNNV2_RNA_RNA004_ADAPTOR (pore 2) / JNNV2_RNA_R9_ADAPTOR, src/jnn.h
// (the constants both pores share: jnn_consts.hpp)
struct AdaptorParams {
    int32_t lo;
    float std_scale;
};
inline AdaptorParams adaptor_params(int pore) { return pore == 2 ? AdaptorParams{500, 0.7f} : AdaptorParams{2000, 0.5f}; }

// event_single(), src/sigfish.c:330-350: pA = ((float)raw + offset) * unit, the three doubles narrowed BEFORE the division
struct RawScale {
    float offset, unit;
};
inline RawScale raw_scale(double digitisation, double offset, double range) {
    const float rangef = static_cast<float>(range), digf = static_cast<float>(digitisation);
    return RawScale{static_cast<float>(offset), rangef / digf};
}

// records a read of len samples can need: each detector closes an event at most every second sample, and one more ends the read
inline int64_t event_capacity(int64_t len) { return len + 2; }

// sfa_query_info_t.status
constexpr int32_t kQueryShort = 1;       // fewer than query_size events: the window is what there is (kept)
constexpr int32_t kQueryDropped = 2;     // the reference ignores the read (et.n = 0)
constexpr int32_t kQueryAutoFailed = 4;  // the automatic start found no adaptor / poly-A tail: kAutoFallback was used
constexpr int kAutoFallback = 50;        // the reference's fallback skip, src/sigfish.c:438-446
constexpr int kMinQuery = 25;            // events a window from the front needs behind its start

struct QueryWindow {
    int64_t start, end;  // events [start, end); 0..0 when the read is not kept
    int32_t status;      // kQuery*
    bool keep;
};

// normalise_single(), src/sigfish.c:433-480.  auto_start (-p -1, from the front only): auto_event is detect_query_start()'s
// event, < 0 when it failed.  A read without events or without samples is not kept and reports nothing.
inline QueryWindow query_window(int64_t n_events, int64_t n_samples, int32_t prefix_size, int32_t query_size, bool from_end, bool auto_start,
                                int64_t auto_event) {
    QueryWindow w{0, 0, 0, n_events > 0 && n_samples > 0};
    if (!w.keep) return w;
    if (!from_end) {  // src/sigfish.c:435-463
        w.start = prefix_size;
        if (auto_start) {
            w.start = auto_event >= 0 ? auto_event : kAutoFallback;
            if (auto_event < 0) w.status |= kQueryAutoFailed;
        }
        w.end = w.start + query_size;
        if (w.start + kMinQuery > n_events) {
            w.start = w.end = 0;
            w.keep = false;
            w.status |= kQueryDropped;
        } else if (w.end > n_events) {
            w.end = n_events;
            w.status |= kQueryShort;
        }
    } else {  // src/sigfish.c:464-478
        w.start = n_events - prefix_size - query_size;
        w.end = n_events - prefix_size;
        if (w.start < 0) {
            w.start = 0;
            w.status |= kQueryShort;
        }
        if (w.end < 0) {
            w.start = w.end = 0;
            w.keep = false;
            w.status |= kQueryDropped;
        }
    }
    return w;
}

}  // namespace sfa
