// events_stream.hpp -- the event detector of events_kernels.hpp as a STREAM, for raw-signal sessions (sfa_session_extend_raw):
// a slot's samples arrive in chunks, its detector state is carried in device memory between the calls, and every event is
// written the moment the peak that closes it fires.  CPU twin: sfa::EventStream (host/events.cpp); both follow detect_events
// operation for operation, so the events equal those of sfa_detect_events over the complete read bit for bit.
//
// Why this can be exact (host/events.cpp, src/events.c:297-508): the prefix sums are sequential double additions -- a carried
// accumulator continues them; with N samples seen and N >= 2 w_long both t-statistics at every position i <= N - w_long need
// sums up to i + w_long <= N only and are not among the positions the batch code zeroes (i > n - w); the peak picker is a
// causal state machine over i; an event needs the sums at its two boundaries.  So the picker walks exactly the positions
// j <= N - w_long as the samples arrive, and the carried state is a constant number of words: a ring of the last 2 w_long + 1
// sums, the two detectors, the sums at each detector's candidate peak and at the open event's start.  At the end of the read
// the remaining positions are walked with the batch code's zeros and the last event runs to the end of the signal.
//
// ev_stream_kernel: one slot per lane, 64 slots per wave, the same recurrence in every lane.  Chunks are staged through LDS
// in tiles of 32 samples with coalesced loads (half a wave per slot, as ev_prefix_kernel does), the rings live in LDS while
// the kernel runs ([index][lane] doubles: a lane's 8-byte access falls on banks 2 * lane, 2 * lane + 1 whatever its index,
// so the 32 lanes of a half never collide although every lane is at another index).  Chunks of one call have different
// lengths: the wave walks to the longest and masks the others.
// ev_stream_norm_kernel: one wave per slot of the call; computes mean and sd over the slot's calibration window once it is
// complete (the two sequential fp32 loops and the double sqrt of sfa_znormalise / ev_query_kernel) and appends the
// normalised means of the new events to the slot's device-resident query, from where the session sweep takes them.  With
// recalibration points (sfa_session_raw_recalibrate, recal_rule.hpp) the window grows with the read: when it does, the
// statistics are computed again over the longer window and the whole query is rewritten, to be swept from event 0.
// In resweep mode (SFA_SESSION_RESWEEP) that is the only way a query is written: nothing is appended, a change of the window
// writes the window's events -- reversed, for RNA without SFA_INV -- and between two changes the query and its row stand.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pre_rules.hpp"  // kAutoFallback, the reference's fallback skip
#include "recal_rule.hpp"

namespace sfa {

constexpr int kEvRing = 29;  // 2 * 14 + 1: the RNA long window (DNA uses 13 of them)

// status bits of a slot: 0..3 are those of sfa_session_raw_info_t and kRawResweep is its bit 4, which belongs to a call (this
// call swept events again that an earlier one had swept) and is never stored in a slot; kRawAnyCut is internal
constexpr int kRawCalibrated = 1, kRawFull = 2, kRawEnded = 4, kRawPoisoned = 8, kRawResweep = 16, kRawAnyCut = 32;

// the carried state of a slot: plain device memory, loaded at the start of a call and stored at its end
struct EvStreamSlot {
    double ring_s[kEvRing], ring_q[kEvRing];  // sum[i], sumsq[i] at i % ring, the last 2 w_long + 1 of them
    double acc, acc2;                         // sum[n], sumsq[n]
    double ps[2], pq[2];                      // sums at the candidate peak of the short / long detector
    double es, eq;                            // sums at the open event's start
    float peak_value[2];
    int32_t masked_to[2], peak_pos[2], valid[2];
    int32_t n, next;                          // samples seen, first position the picker has not walked
    int32_t ev_start, n_events;               // start of the open event, final events written
    int32_t status, q_done;                   // kRaw* bits; events of the query normalised so far
    float mean, sd;                           // frozen at calibration
};
static_assert(sizeof(EvStreamSlot) == 592, "sfa_session_raw_bytes documents 592 bytes of detector state per slot");

struct EvRecord {  // sfa_event_t
    uint64_t start;
    float length, mean, stdv;
    uint32_t pad;
};
static_assert(sizeof(EvRecord) == 24, "layout of sfa_event_t");

constexpr int kEntryFresh = 1, kEntryEnd = 2;  // e_flags: first chunk after a reset (the state is initialised); end of the read

struct EvStreamArgs {
    const int16_t *raw;       // the call's samples, concatenated
    const int64_t *raw_off;   // [n + 1]
    const int32_t *slot;      // [n]
    const int32_t *e_flags;   // [n] kEntry*
    const float *scale;       // [n][2] offset, raw_unit = range / digitisation in fp32 (event_single)
    EvStreamSlot *state;      // [n_slots]
    EvRecord *events;         // [n_slots][ev_cap] final events, means in pA
    int32_t n, ev_cap;        // ev_cap = skip + query: the detector stops there
    int32_t w1, w2;
    float thr1, thr2, peak_height;
};

constexpr int kStreamTile = 32;

__global__ void __launch_bounds__(64) ev_stream_kernel(const EvStreamArgs a);

#ifdef SFA_DEFINE_SESSION_KERNELS  // the plain kernel: defined in exactly one translation unit (sfa_session.hip), as sdtw_session.hpp's
__global__ void __launch_bounds__(64) ev_stream_kernel(const EvStreamArgs a) {
    __shared__ double ring_s[kEvRing][64];
    __shared__ double ring_q[kEvRing][64];
    __shared__ float raw_t[64][kStreamTile + 1];
    __shared__ uint32_t lds_rel[64];
    __shared__ int32_t lds_len[64];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * 64 + lane;
    const bool live = i < a.n;
    const int ring = 2 * a.w2 + 1;
    const int64_t b0 = a.raw_off[blockIdx.x * 64];  // (the block's first entry exists)
    const int64_t b = a.raw_off[live ? i : a.n];
    const int32_t len = live ? static_cast<int32_t>(a.raw_off[i + 1] - b) : 0;
    const int ef = live ? a.e_flags[i] : 0;
    const float off = live ? a.scale[2 * i] : 0.0f, unit = live ? a.scale[2 * i + 1] : 0.0f;
    EvStreamSlot *st = a.state + (live ? a.slot[i] : 0);
    EvRecord *evs = a.events + static_cast<int64_t>(live ? a.slot[i] : 0) * a.ev_cap;
    lds_rel[lane] = static_cast<uint32_t>(b - b0);
    lds_len[lane] = len;

    // ---- the carried state ----
    const bool fresh = !live || (ef & kEntryFresh);
    double acc = 0.0, acc2 = 0.0, ps0 = 0.0, pq0 = 0.0, ps1 = 0.0, pq1 = 0.0, es = 0.0, eq = 0.0;
    float pv0 = 3.402823466e+38f, pv1 = 3.402823466e+38f;
    int mt0 = 0, mt1 = 0, pp0 = -1, pp1 = -1, vp0 = 0, vp1 = 0;
    int n = 0, next = 0, ev_start = 0, nev = 0, status = 0, q_done = 0;
    float mean = 0.0f, sd = 0.0f;
    if (!fresh) {
        acc = st->acc, acc2 = st->acc2;
        ps0 = st->ps[0], ps1 = st->ps[1], pq0 = st->pq[0], pq1 = st->pq[1];
        es = st->es, eq = st->eq;
        pv0 = st->peak_value[0], pv1 = st->peak_value[1];
        mt0 = st->masked_to[0], mt1 = st->masked_to[1];
        pp0 = st->peak_pos[0], pp1 = st->peak_pos[1];
        vp0 = st->valid[0], vp1 = st->valid[1];
        n = st->n, next = st->next, ev_start = st->ev_start, nev = st->n_events, status = st->status, q_done = st->q_done;
        mean = st->mean, sd = st->sd;
    }
    for (int r = 0; r < ring; ++r) {
        ring_s[r][lane] = fresh ? 0.0 : st->ring_s[r];
        ring_q[r][lane] = fresh ? 0.0 : st->ring_q[r];
    }
    int ri = n % ring;  // index of sum[n]
    const bool was_ended = (status & kRawEnded) != 0;
    const bool end = (ef & kEntryEnd) != 0;

    // the ring entry of sum[p], n - p <= 2 w_long
    auto at = [&](int p) {
        int x = ri - (n - p);
        return x < 0 ? x + ring : x;
    };
    // tstat()[p] of a signal of n samples so far: compute_tstat(), src/events.c:319-368
    auto tstat = [&](int w, int p) -> float {
        if (n < 2 * w || p < w || p > n - w) return 0.0f;
        const float wf = static_cast<float>(w);
        const int xp = at(p), xh = at(p + w);
        double s1 = ring_s[xp][lane], q1 = ring_q[xp][lane];
        if (p > w) {
            const int xl = at(p - w);
            s1 -= ring_s[xl][lane];
            q1 -= ring_q[xl][lane];
        }
        const float s2 = static_cast<float>(ring_s[xh][lane] - ring_s[xp][lane]);
        const float q2 = static_cast<float>(ring_q[xh][lane] - ring_q[xp][lane]);
        const float mean1 = static_cast<float>(s1 / static_cast<double>(wf));
        const float mean2 = s2 / wf;
        double cv = q1 / static_cast<double>(wf);
        cv -= static_cast<double>(mean1 * mean1);
        cv += static_cast<double>(q2 / wf);
        cv -= static_cast<double>(mean2 * mean2);
        float combined = static_cast<float>(cv);
        combined = fmaxf(combined, 1.17549435e-38f);  // FLT_MIN
        const float delta = mean2 - mean1;
        return static_cast<float>(fabs(static_cast<double>(delta)) / sqrt(static_cast<double>(combined / wf)));
    };
    // create_event(), src/events.c:461-477, for [ev_start, end_pos) with the sums at both ends
    auto emit = [&](int end_pos, double s1, double q1) {
        if (nev < a.ev_cap) {
            EvRecord e;
            e.start = static_cast<uint64_t>(ev_start);
            e.length = static_cast<float>(static_cast<uint64_t>(end_pos - ev_start));
            e.mean = static_cast<float>(s1 - es) / e.length;
            const float dsq = static_cast<float>(q1 - eq);
            const float var = dsq / e.length - e.mean * e.mean;
            e.stdv = sqrtf(fmaxf(var, 0.0f));
            e.pad = 0;
            evs[nev] = e;
            ++nev;
        }
    };
    // one detector at position p (short_long_peak_detector(), src/events.c:375-458); K = 0 short, 1 long
    auto detector = [&](const int K, int p, double sp, double qp, int &mt, int &pp, float &pv, int &vp, double &dps, double &dpq) {
        if (mt >= p) return;
        const int w = K ? a.w2 : a.w1;
        const float threshold = K ? a.thr2 : a.thr1;
        const float cur = tstat(w, p);
        if (pp == -1) {
            if (cur < pv) {
                pv = cur;
            } else if (cur - pv > a.peak_height) {
                pv = cur;
                pp = p;
                dps = sp;
                dpq = qp;
            }
        } else {
            if (cur > pv) {
                pv = cur;
                pp = p;
                dps = sp;
                dpq = qp;
            }
            if (K == 0 && pv > threshold) {  // the short detector masks the long one
                mt1 = pp + w;
                pp1 = -1;
                pv1 = 3.402823466e+38f;
                vp1 = 0;
            }
            if (pv - cur > a.peak_height && pv > threshold) vp = 1;
            if (vp && (p - pp) > w / 2) {
                emit(pp, dps, dpq);  // the peak closes the open event and opens the next
                ev_start = pp;
                es = dps;
                eq = dpq;
                status |= kRawAnyCut;
                pp = -1;
                pv = cur;
                vp = 0;
            }
        }
    };

    int maxlen = len + (end ? 1 : 0);  // the step behind the last sample is the end of the read
    for (int o = 32; o; o >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, o));
    __syncthreads();
    const int half = lane >> 5, jl = lane & 31;
    const int16_t *rawp = a.raw + b0;
    for (int base = 0; base < maxlen; base += kStreamTile) {
        // coalesced: 32 consecutive samples of one slot's chunk per half-wave
        for (int it = 0; it < 32; ++it) {
            const int r = 2 * it + half;
            const int bj = base + jl;
            raw_t[r][jl] = bj < lds_len[r] ? static_cast<float>(rawp[lds_rel[r] + static_cast<uint32_t>(bj)]) : 0.0f;
        }
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < kStreamTile; ++jj) {
            const int j = base + jj;
            const bool samp = j < len && !was_ended && nev < a.ev_cap;  // a full slot's detector has stopped
            const bool fin = j == len && end && !was_ended;
            if (samp || fin) {
                int hi = -1;
                if (samp) {
                    const float pa = (raw_t[lane][jj] + off) * unit;
                    const float sq = pa * pa;
                    acc = acc + static_cast<double>(pa);
                    acc2 = acc2 + static_cast<double>(sq);
                    ++n;
                    ri = ri + 1 == ring ? 0 : ri + 1;
                    ring_s[ri][lane] = acc;
                    ring_q[ri][lane] = acc2;
                    if (n >= 2 * a.w2) hi = n - a.w2;
                } else if (nev < a.ev_cap) {
                    hi = n - 1;  // the positions the batch code walks with zeros past n - w
                }
                for (int p = next; p <= hi; ++p) {  // one position per sample once N >= 2 w_long
                    const int xp = at(p);
                    const double sp = ring_s[xp][lane], qp = ring_q[xp][lane];
                    detector(0, p, sp, qp, mt0, pp0, pv0, vp0, ps0, pq0);
                    detector(1, p, sp, qp, mt1, pp1, pv1, vp1, ps1, pq1);
                }
                if (hi >= next) next = hi + 1;
                if (fin) {
                    if (status & kRawAnyCut) emit(n, acc, acc2);  // the last event runs to the end of the signal
                    status |= kRawEnded;
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (nev >= a.ev_cap) status |= kRawFull;
    st->acc = acc, st->acc2 = acc2;
    st->ps[0] = ps0, st->ps[1] = ps1, st->pq[0] = pq0, st->pq[1] = pq1;
    st->es = es, st->eq = eq;
    st->peak_value[0] = pv0, st->peak_value[1] = pv1;
    st->masked_to[0] = mt0, st->masked_to[1] = mt1;
    st->peak_pos[0] = pp0, st->peak_pos[1] = pp1;
    st->valid[0] = vp0, st->valid[1] = vp1;
    st->n = n, st->next = next, st->ev_start = ev_start, st->n_events = nev, st->status = status, st->q_done = q_done;
    st->mean = mean, st->sd = sd;
    for (int r = 0; r < ring; ++r) {
        st->ring_s[r] = ring_s[r][lane];
        st->ring_q[r] = ring_q[r][lane];
    }
}
#endif

// what a call brings back to the host per slot: counts and the normalisation the slot has now
struct EvStreamOut {
    int32_t n_events, q_first, q_new, status;  // status: bits 0..3 of the slot | kRawResweep for this call
    float mean, sd;
    int32_t window, pad;                       // events the mean and sd span (0: not calibrated)
};

// status of a slot's automatic start: the low nibble is the state, kAutoAtFinal says the target was frozen (or given up) at
// the slot's final point (sfa_session_auto_t.status)
constexpr int kAutoPending = 0, kAutoResolved = 1, kAutoNoTarget = 2, kAutoNoEvent = 3, kAutoBeyondMax = 4, kAutoAtFinal = 16;
constexpr int32_t kAutoMaxSamples = 1 << 20;      // 1200 x 2^20 < 2^31: the prefix sums of a slot fit 32 bits

struct EvAutoSlot {   // per slot, device memory; sfa_session_auto_t is made of it
    int32_t target;     // frozen target sample, -1 before
    int32_t skip;       // resolved skip, -1 before
    int32_t frozen_at;  // the point N_k at which the target was frozen (or the final point that gave none), 0 before
    int32_t status;     // kAuto*
};

// what ev_stream_norm_kernel does for a session with the automatic start before anything else: the slot's skip.  Block-uniform.
// A frozen target is resolved to the first final event whose start is >= target (starts ascend, so the binary search equals the
// reference's walk) in the call in which that event is in the table; *au is updated where something changed.
__device__ __forceinline__ bool auto_resolve(EvAutoSlot *au, const EvRecord *ev, int nev, int ev_cap, int max_skip, bool ended) {
    if (au->skip >= 0 || au->target < 0) return false;
    const uint64_t target = static_cast<uint64_t>(au->target);
    int lo = 0, hi = nev;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ev[mid].start < target) lo = mid + 1;
        else hi = mid;
    }
    if (lo < nev && lo <= max_skip) {
        au->skip = lo;
        au->status = (au->status & ~15) | kAutoResolved;
    } else if (lo < nev || nev >= ev_cap) {  // the table is full below the target: the event would lie beyond it
        au->skip = kAutoFallback;
        au->status = (au->status & ~15) | kAutoBeyondMax;
    } else if (ended) {
        au->skip = kAutoFallback;
        au->status = (au->status & ~15) | kAutoNoEvent;
    } else {
        return false;
    }
    return true;
}

struct EvNormArgs {
    const int32_t *slot;     // [n]
    EvStreamSlot *state;
    int32_t *window;         // [n_slots] W_cur, the window a calibrated slot's normalisation spans: a side array of the session,
                             // since EvStreamSlot keeps its 592 bytes; it means something only while kRawCalibrated is set
    const EvRecord *events;  // [n_slots][ev_cap]
    float *query;            // [n_slots][query] the slots' normalised queries
    EvStreamOut *out;        // [n]
    uint8_t *bad;            // [n] the slot is poisoned: not swept
    int32_t n, ev_cap, skip, norm, query_cap;
    int32_t n_at;            // recalibration points (recal_rule.hpp); 0 and no flags: the window is frozen at norm
    uint32_t flags;          // kRecalAtEnd
    int32_t at[kRecalMaxPoints];
    int32_t resweep;         // SFA_SESSION_RESWEEP: the query is the window's W events, written only when W changes
    int32_t reversed;        // (with resweep) q[i] = z(event[skip + W - 1 - i]): SFA_RNA without SFA_INV
};

// the second argument of ev_stream_norm_kernel: read by the <true> instantiation only (automatic query start), so that the
// argument block and the code of the <false> one stay what they were.  EvNormArgs.skip is then the largest skip a slot may resolve
struct EvNormAutoArgs {
    EvAutoSlot *state;  // [n_slots] the slots' targets and skips
    EvAutoSlot *out;    // [n] what the call's slots hold after it
};

constexpr int kNormTile = 2048;  // pA means staged per tile of the statistics: 8 KB of LDS

// One wave per slot of the call.  The window W the slot must have now follows from its counts (recal_window).  Where it differs
// from the window its normalisation spans -- the first calibration is the case W_cur = 0 -- mean and sd are computed over events
// [skip, skip + W): all lanes stage the window's pA means from the 24-byte records into LDS, tile by tile, and lane 0 runs
// sfa_znormalise's two sequential fp32 loops over them (so the result is the host's bit for bit); then all lanes rewrite the
// WHOLE query [0, q_avail) and the host sweeps it as a first chunk.  Otherwise the new events are appended as before.
// Resweep mode (a.resweep, block-uniform like a.reversed): no append.  A change of W writes q[0, W) -- lane l stores q[i] from
// record skip + i, or skip + W - 1 - i when reversed: consecutive lanes still read consecutive records -- and reports q_first = 0,
// q_new = W; any other call reports q_new = 0 and leaves q_done = W.  Events beyond skip + W wait in the table for the next point.
//
// AUTO (sfa_session_raw_auto_start): the slot's skip is its own.  It is resolved here first (auto_resolve), and until it is the
// slot has no query: q_avail = 0, not calibrated.  Everything behind that is the rule above with the slot's skip in place of
// a.skip, and "full" is n_events >= skip + query.  The instantiation without AUTO is the kernel as it was.
template <bool AUTO>
__global__ void __launch_bounds__(64) ev_stream_norm_kernel(const EvNormArgs a, const EvNormAutoArgs x) {
    __shared__ float tile[kNormTile];
    __shared__ float stat[2];
    __shared__ int s_status;
    const int i = blockIdx.x, lane = threadIdx.x;
    const int slot = a.slot[i];
    EvStreamSlot *st = a.state + slot;
    const EvRecord *ev = a.events + static_cast<int64_t>(slot) * a.ev_cap;
    const int nev = st->n_events, q_done = st->q_done;
    int status = st->status;
    float mean = st->mean, sd = st->sd;
    EvAutoSlot au{};
    bool au_changed = false;
    if constexpr (AUTO) {
        au = x.state[slot];
        au_changed = auto_resolve(&au, ev, nev, a.ev_cap, a.skip, (status & kRawEnded) != 0);
    }
    const int q_avail = (AUTO && au.skip < 0) ? 0 : recal_q_avail(nev, AUTO ? au.skip : a.skip, a.query_cap);
    const int w_cur = (status & kRawCalibrated) ? a.window[slot] : 0;
    int w = w_cur;
    if (!(status & kRawPoisoned))  // (a poisoned slot keeps what poisoned it until it is reset)
        w = max(w_cur, recal_window(q_avail, (status & kRawEnded) != 0, a.norm, a.query_cap, a.at, a.n_at, a.flags));
    const bool recal = w != w_cur;  // (block-uniform, as everything above)
    if (recal) {
        const float cnt = static_cast<float>(w);
        float m = 0.0f, var = 0.0f;  // lane 0's
        for (int pass = 0; pass < 2; ++pass) {
            for (int base = 0; base < w; base += kNormTile) {
                const int len = min(kNormTile, w - base);
                for (int j = lane; j < len; j += 64) tile[j] = ev[(AUTO ? au.skip : a.skip) + base + j].mean;
                __syncthreads();
                if (lane == 0) {  // sfa_znormalise's sums, in its order
                    if (pass == 0) {
                        for (int j = 0; j < len; ++j) m += tile[j];
                    } else {
                        for (int j = 0; j < len; ++j) {
                            const float dv = tile[j] - m;
                            var += dv * dv;
                        }
                    }
                }
                __syncthreads();
            }
            if (pass == 0) m /= cnt;
        }
        if (lane == 0) {
            var /= cnt;
            stat[0] = m;
            stat[1] = static_cast<float>(sqrt(static_cast<double>(var)));
        }
        __syncthreads();
        mean = stat[0];
        sd = stat[1];
        status |= kRawCalibrated;
        if (!(sd > 0.0f) || sd > 3.402823466e+38f) status |= kRawPoisoned;  // zero, NaN or inf: no query can be made of it
    }
    const int q_first = recal ? 0 : q_done;
    const int q_end = a.resweep ? (recal ? w : q_first) : q_avail;  // one behind the last query event this call writes
    const int q_top = a.reversed ? q_end - 1 : 0;                   // reversed: the event that goes to q[0]
    int q_new = 0;
    if (lane == 0) s_status = 0;
    __syncthreads();
    if ((status & kRawCalibrated) && !(status & kRawPoisoned)) {
        q_new = q_end - q_first;
        float *q = a.query + static_cast<int64_t>(slot) * a.query_cap;
        bool bad = false;
        for (int e = q_first + lane; e < q_end; e += 64) {
            const float v = (ev[(AUTO ? au.skip : a.skip) + (a.reversed ? q_top - e : e)].mean - mean) / sd;
            q[e] = v;
            bad = bad || !(fabsf(v) <= 3.402823466e+38f);
        }
        if (bad) s_status = kRawPoisoned;  // (every writer writes the same value)
    }
    __syncthreads();
    status |= s_status;
    if (status & kRawPoisoned) q_new = 0;
    if (lane == 0) {
        st->status = status;
        st->mean = mean;
        st->sd = sd;
        if (!(status & kRawPoisoned)) st->q_done = q_first + q_new;
        a.window[slot] = w;
        EvStreamOut o;
        o.n_events = nev;
        o.q_first = (status & kRawPoisoned) ? q_done : q_first;
        o.q_new = q_new;
        o.status = (status & 15) | ((recal && q_done > 0 && q_new > 0) ? kRawResweep : 0);
        if constexpr (AUTO) {
            o.status &= ~kRawFull;  // (the detector's bit means the TABLE is full; a slot is full at skip + query events)
            if (au.skip >= 0 && nev >= au.skip + a.query_cap) o.status |= kRawFull;
            if (au_changed) x.state[slot] = au;
            x.out[i] = au;
        }
        o.mean = mean;
        o.sd = sd;
        o.window = w;
        o.pad = 0;
        a.out[i] = o;
        a.bad[i] = (status & kRawPoisoned) ? 1 : 0;
    }
}

// sfa_session_query_span: the raw coordinates of a slot's query, gathered from its event table.  One lane per named slot, two
// records each; q_events comes from the host (0: the slot is not calibrated, or has been reset since -- its table is stale).
struct EvSpanArgs {
    const int32_t *slot;     // [n]
    const int32_t *q_events; // [n] query events swept
    const EvRecord *events;  // [n_slots][ev_cap]
    uint64_t *span;          // [n][2] start of event skip | start + length of event skip + q_events - 1
    int32_t n, ev_cap, skip, query_cap;
    const int32_t *skips;    // [n] PER_SLOT only (automatic query start): each slot's own skip in place of `skip`
};

template <bool PER_SLOT>
__global__ void __launch_bounds__(64) ev_query_span_kernel(const EvSpanArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n) return;
    const int q = min(a.q_events[i], a.query_cap);
    uint64_t first = 0, last = 0;
    if (q > 0) {
        const EvRecord *ev = a.events + static_cast<int64_t>(a.slot[i]) * a.ev_cap + (PER_SLOT ? a.skips[i] : a.skip);
        first = ev[0].start;
        last = ev[q - 1].start + static_cast<uint64_t>(ev[q - 1].length);
    }
    a.span[2 * i] = first;
    a.span[2 * i + 1] = last;
}

}  // namespace sfa
