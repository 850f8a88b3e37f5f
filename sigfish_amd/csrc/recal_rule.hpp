// recal_rule.hpp -- over which window a raw-session slot is normalised (sfa_session_raw_recalibrate): ONE pure function for the
// device (events_stream.hpp, ev_stream_norm_kernel), the library's checks (sfa_session.hip), the command line (cli/options.cpp)
// and tests/c/recal_window.cpp.  Python twin: sigfish_amd.api.recal_window / recal_double.
//
// A slot has q_avail = min(n_events - skip, query) query events (0 below skip) and has seen its end of read or not.  The window
// length W -- mean and sd span events [skip, skip + W) -- is
//   q_avail                      with kRecalAtEnd, once ended, when 25 <= q_avail < query: the reference's "too short" window
//                                (normalise_single, src/sigfish.c:450-461)
//   the largest at[k] <= q_avail otherwise, if there is one
//   norm                         otherwise, if q_avail >= norm
//   0                            otherwise: not calibrated
// at[] ascends and norm < at[0], at[n_at - 1] <= query, so W never shrinks while a slot grows: q_avail only grows, and a slot that
// ends keeps its q_avail, which is no smaller than any point it has passed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SFA_RECAL_HD __host__ __device__
#else
#define SFA_RECAL_HD
#endif

namespace sfa {

constexpr int32_t kRecalMaxPoints = 32;
constexpr uint32_t kRecalAtEnd = 0x1;  // SFA_RECAL_AT_END
constexpr int32_t kRecalMinQuery = 25; // the reference's minimum query

SFA_RECAL_HD inline int32_t recal_q_avail(int32_t n_events, int32_t skip, int32_t query) {
    const int32_t q = n_events - skip;
    return q < 0 ? 0 : (q < query ? q : query);
}

SFA_RECAL_HD inline int32_t recal_window(int32_t q_avail, bool ended, int32_t norm, int32_t query, const int32_t *at, int32_t n_at, uint32_t flags) {
    if ((flags & kRecalAtEnd) && ended && q_avail >= kRecalMinQuery && q_avail < query) return q_avail;
    int32_t w = 0;
    for (int32_t k = 0; k < n_at; ++k)
        if (at[k] <= q_avail) w = at[k];
    if (w > 0) return w;
    return q_avail >= norm ? norm : 0;
}

// what a list must satisfy: norm < at[0] < ... < at[n_at - 1] <= query, at most kRecalMaxPoints of them.  nullptr: it does
inline const char *recal_list_error(const int32_t *at, int64_t n_at, int32_t norm, int32_t query) {
    if (n_at < 0 || (n_at > 0 && !at)) return "a negative count or a null list";
    if (n_at > kRecalMaxPoints) return "more than 32 points";
    for (int64_t k = 0; k < n_at; ++k) {
        if (k == 0 && at[k] <= norm) return "the first point must lie above the calibration window (norm)";
        if (k > 0 && at[k] <= at[k - 1]) return "the points must ascend strictly";
        if (at[k] > query) return "a point lies above the query size";
    }
    return nullptr;
}

// "double": 2 norm, 4 norm, ... below query, then query itself; nothing when norm == query (no longer window exists).
// Writes at most kRecalMaxPoints points (every shape sfa_session_raw_config accepts gives at most 27) and returns their number.
inline int32_t recal_double(int32_t norm, int32_t query, int32_t *at) {
    int32_t n = 0;
    if (norm < 1 || norm >= query) return 0;
    for (int64_t w = 2 * static_cast<int64_t>(norm); w < query && n < kRecalMaxPoints - 1; w *= 2) at[n++] = static_cast<int32_t>(w);
    at[n++] = query;
    return n;
}

}  // namespace sfa
