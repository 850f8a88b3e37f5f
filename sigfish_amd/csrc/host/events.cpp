// events.cpp -- see events.hpp.  Compiled with -ffp-contract=off: the reference is built by gcc -O2 -std=c99
// for x86-64 (no FMA contraction, float expressions evaluated in float, FLT_EVAL_METHOD 0).
#include "events.hpp"

#include "../jnn_consts.hpp"
#include "../pre_rules.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace sfa {

void raw_to_picoamps(const int16_t *raw, int64_t n, double digitisation, double offset, double range, float *out) {
    const RawScale sc = raw_scale(digitisation, offset, range);
    for (int64_t i = 0; i < n; ++i) out[i] = (static_cast<float>(raw[i]) + sc.offset) * sc.unit;
}

namespace {

// windowed two-sample t statistic from prefix sums, src/events.c:319-368
std::vector<float> tstat(const std::vector<double> &sum, const std::vector<double> &sumsq, size_t n, size_t w) {
    std::vector<float> t(n, 0.0f);
    if (n < 2 * w || w < 2) return t;
    const float wf = static_cast<float>(w);
    for (size_t i = w; i <= n - w; ++i) {
        double s1 = sum[i], q1 = sumsq[i];
        if (i > w) {
            s1 -= sum[i - w];
            q1 -= sumsq[i - w];
        }
        const float s2 = static_cast<float>(sum[i + w] - sum[i]);
        const float q2 = static_cast<float>(sumsq[i + w] - sumsq[i]);
        const float mean1 = static_cast<float>(s1 / static_cast<double>(wf));
        const float mean2 = s2 / wf;
        // double accumulation, left to right, exactly as the mixed-type C expression promotes
        double cv = q1 / static_cast<double>(wf);
        cv -= static_cast<double>(mean1 * mean1);
        cv += static_cast<double>(q2 / wf);
        cv -= static_cast<double>(mean2 * mean2);
        float combined = static_cast<float>(cv);
        combined = std::fmax(combined, FLT_MIN);
        const float delta = mean2 - mean1;
        t[i] = static_cast<float>(std::fabs(static_cast<double>(delta)) / std::sqrt(static_cast<double>(combined / wf)));
    }
    return t;
}

struct Detector {  // src/events.c:281-293
    const float *signal;
    float threshold;
    size_t window;
    size_t masked_to = 0;
    int peak_pos = -1;
    float peak_value = FLT_MAX;
    bool valid_peak = false;
};

// short/long detector interplay, src/events.c:375-458
std::vector<size_t> pick_peaks(Detector &sd, Detector &ld, size_t n, float peak_height) {
    std::vector<size_t> peaks;
    Detector *det[2] = {&sd, &ld};
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 2; ++k) {
            Detector &d = *det[k];
            if (d.masked_to >= i) continue;
            const float cur = d.signal[i];
            if (d.peak_pos == -1) {
                if (cur < d.peak_value) {
                    d.peak_value = cur;  // deeper minimum
                } else if (cur - d.peak_value > peak_height) {
                    d.peak_value = cur;  // a qualifying rise: start tracking a peak
                    d.peak_pos = static_cast<int>(i);
                }
            } else {
                if (cur > d.peak_value) {
                    d.peak_value = cur;
                    d.peak_pos = static_cast<int>(i);
                }
                if (k == 0 && d.peak_value > d.threshold) {  // the short detector masks the long one
                    ld.masked_to = d.peak_pos + d.window;
                    ld.peak_pos = -1;
                    ld.peak_value = FLT_MAX;
                    ld.valid_peak = false;
                }
                if (d.peak_value - cur > peak_height && d.peak_value > d.threshold) d.valid_peak = true;
                if (d.valid_peak && (i - static_cast<size_t>(d.peak_pos)) > d.window / 2) {
                    peaks.push_back(static_cast<size_t>(d.peak_pos));
                    d.peak_pos = -1;
                    d.peak_value = cur;
                    d.valid_peak = false;
                }
            }
        }
    }
    return peaks;
}

sfa_event_t make_event(size_t start, size_t end, const std::vector<double> &sum, const std::vector<double> &sumsq) {
    sfa_event_t e;  // src/events.c:461-477
    e.start = start;
    e.length = static_cast<float>(end - start);
    e.mean = static_cast<float>(sum[end] - sum[start]) / e.length;
    const float dsq = static_cast<float>(sumsq[end] - sumsq[start]);
    const float var = dsq / e.length - e.mean * e.mean;
    e.stdv = std::sqrt(std::fmax(var, 0.0f));
    return e;
}

}  // namespace

std::vector<sfa_event_t> detect_events(const float *pa, int64_t n_, bool rna) {
    std::vector<sfa_event_t> out;
    if (n_ <= 0) return out;
    const size_t n = static_cast<size_t>(n_);
    const DetectorParams p = detector_params(rna);
    const size_t w1 = static_cast<size_t>(p.w1), w2 = static_cast<size_t>(p.w2);
    // prefix sums in double; the square is a FLOAT product promoted afterwards (src/events.c:297-307)
    std::vector<double> sum(n + 1), sumsq(n + 1);
    sum[0] = 0.0;
    sumsq[0] = 0.0;
    for (size_t i = 0; i < n; ++i) {
        sum[i + 1] = sum[i] + static_cast<double>(pa[i]);
        sumsq[i + 1] = sumsq[i] + static_cast<double>(pa[i] * pa[i]);
    }
    const std::vector<float> t1 = tstat(sum, sumsq, n, w1), t2 = tstat(sum, sumsq, n, w2);
    Detector sd{t1.data(), p.thr1, w1}, ld{t2.data(), p.thr2, w2};
    std::vector<size_t> peaks = pick_peaks(sd, ld, n, p.peak_height);
    // create_events(), src/events.c:479-508: peaks equal to 0 or >= n do not open an event
    std::vector<size_t> cuts;
    for (size_t pk : peaks)
        if (pk > 0 && pk < n) cuts.push_back(pk);
    // the reference indexes the raw peak list positionally; a peak at 0 cannot occur (tstat[0..w) is zero)
    if (cuts.empty()) return out;  // the reference reads out of bounds here; treat as "no events"
    out.reserve(cuts.size() + 1);
    out.push_back(make_event(0, cuts[0], sum, sumsq));
    for (size_t e = 1; e < cuts.size(); ++e) out.push_back(make_event(cuts[e - 1], cuts[e], sum, sumsq));
    out.push_back(make_event(cuts.back(), n, sum, sumsq));
    return out;
}

// ---------------------------------------------------------------------------------------------------------
// the detector as a stream (events.hpp); every expression is the one of tstat / pick_peaks / make_event above
// ---------------------------------------------------------------------------------------------------------
EventStream::EventStream(double digitisation, double offset, double range, bool rna) {
    const DetectorParams p = detector_params(rna);
    w1_ = p.w1;
    w2_ = p.w2;
    ring_ = 2 * w2_ + 1;
    thr1_ = p.thr1;
    thr2_ = p.thr2;
    peak_height_ = p.peak_height;
    const RawScale sc = raw_scale(digitisation, offset, range);  // raw_to_picoamps()
    offf_ = sc.offset;
    unit_ = sc.unit;
    for (int i = 0; i < kRing; ++i) st_.ring_s[i] = st_.ring_q[i] = 0.0;  // (sum[0] = sumsq[0] = 0)
}

namespace {

// tstat()[i] of a signal of n samples (so far: any n >= i + w gives the same value) from the ring
float tstat_ring(const EventStream::State &s, int ring, int64_t n, int w, int64_t i) {
    if (n < 2 * w || i < w || i > n - w) return 0.0f;
    const float wf = static_cast<float>(w);
    double s1 = s.ring_s[i % ring], q1 = s.ring_q[i % ring];
    if (i > w) {
        s1 -= s.ring_s[(i - w) % ring];
        q1 -= s.ring_q[(i - w) % ring];
    }
    const float s2 = static_cast<float>(s.ring_s[(i + w) % ring] - s.ring_s[i % ring]);
    const float q2 = static_cast<float>(s.ring_q[(i + w) % ring] - s.ring_q[i % ring]);
    const float mean1 = static_cast<float>(s1 / static_cast<double>(wf));
    const float mean2 = s2 / wf;
    double cv = q1 / static_cast<double>(wf);
    cv -= static_cast<double>(mean1 * mean1);
    cv += static_cast<double>(q2 / wf);
    cv -= static_cast<double>(mean2 * mean2);
    float combined = static_cast<float>(cv);
    combined = std::fmax(combined, FLT_MIN);
    const float delta = mean2 - mean1;
    return static_cast<float>(std::fabs(static_cast<double>(delta)) / std::sqrt(static_cast<double>(combined / wf)));
}

sfa_event_t stream_event(int64_t start, int64_t end, double s0, double q0, double s1, double q1) {  // make_event()
    sfa_event_t e;
    e.start = static_cast<uint64_t>(start);
    e.length = static_cast<float>(static_cast<size_t>(end - start));
    e.mean = static_cast<float>(s1 - s0) / e.length;
    const float dsq = static_cast<float>(q1 - q0);
    const float var = dsq / e.length - e.mean * e.mean;
    e.stdv = std::sqrt(std::fmax(var, 0.0f));
    return e;
}

}  // namespace

// pick_peaks() over the positions [s.next, upto] of a signal that has n_final samples (while the read goes on: any value
// >= upto + w_long); a peak closes the open event at once.  Returns emitted + the events made; those below cap are written.
int64_t EventStream::walk(State &s, int64_t upto, int64_t n_final, sfa_event_t *out, int64_t cap, int64_t emitted) const {
    for (int64_t i = s.next; i <= upto; ++i) {
        const double si = s.ring_s[i % ring_], qi = s.ring_q[i % ring_];
        for (int k = 0; k < 2; ++k) {
            Det &d = s.det[k];
            if (d.masked_to >= i) continue;
            const int w = k ? w2_ : w1_;
            const float threshold = k ? thr2_ : thr1_;
            const float cur = tstat_ring(s, ring_, n_final, w, i);
            if (d.peak_pos == -1) {
                if (cur < d.peak_value) {
                    d.peak_value = cur;
                } else if (cur - d.peak_value > peak_height_) {
                    d.peak_value = cur;
                    d.peak_pos = i;
                    d.ps = si;
                    d.pq = qi;
                }
            } else {
                if (cur > d.peak_value) {
                    d.peak_value = cur;
                    d.peak_pos = i;
                    d.ps = si;
                    d.pq = qi;
                }
                if (k == 0 && d.peak_value > threshold) {
                    Det &ld = s.det[1];
                    ld.masked_to = d.peak_pos + w;
                    ld.peak_pos = -1;
                    ld.peak_value = FLT_MAX;
                    ld.valid_peak = false;
                }
                if (d.peak_value - cur > peak_height_ && d.peak_value > threshold) d.valid_peak = true;
                if (d.valid_peak && (i - d.peak_pos) > w / 2) {
                    // create_events(): a peak inside (0, n) closes the open event (a walked position is always < n, and a
                    // candidate is never at 0: position 0 is masked)
                    if (emitted < cap) out[emitted] = stream_event(s.ev_start, d.peak_pos, s.es, s.eq, d.ps, d.pq);
                    ++emitted;
                    s.ev_start = d.peak_pos;
                    s.es = d.ps;
                    s.eq = d.pq;
                    s.any_cut = true;
                    d.peak_pos = -1;
                    d.peak_value = cur;
                    d.valid_peak = false;
                }
            }
        }
    }
    if (upto >= s.next) s.next = upto + 1;
    return emitted;
}

int64_t EventStream::push(const int16_t *raw, int64_t n, sfa_event_t *out, int64_t cap) {
    if (st_.finished) return -1;
    State s = st_;  // committed only when everything fits
    int64_t emitted = 0;
    for (int64_t j = 0; j < n; ++j) {
        const float pa = (static_cast<float>(raw[j]) + offf_) * unit_;
        s.acc = s.acc + static_cast<double>(pa);
        s.acc2 = s.acc2 + static_cast<double>(pa * pa);
        ++s.n;
        s.ring_s[s.n % ring_] = s.acc;
        s.ring_q[s.n % ring_] = s.acc2;
        if (s.n >= 2 * w2_) emitted = walk(s, s.n - w2_, s.n, out, cap, emitted);
    }
    if (emitted > cap) return emitted;
    st_ = s;
    return emitted;
}

int64_t EventStream::finish(sfa_event_t *out, int64_t cap) {
    if (st_.finished) return -1;
    State s = st_;
    int64_t emitted = walk(s, s.n - 1, s.n, out, cap, 0);
    if (s.any_cut) {  // the last event runs to the end of the signal; no peak at all: no events
        if (emitted < cap) out[emitted] = stream_event(s.ev_start, s.n, s.es, s.eq, s.acc, s.acc2);
        ++emitted;
    }
    if (emitted > cap) return emitted;
    s.finished = true;
    st_ = s;
    return emitted;
}

// ---------------------------------------------------------------------------------------------------------
// adaptor / poly-A segmenters (src/jnn.c), only reached with RNA and -p -1
// ---------------------------------------------------------------------------------------------------------
namespace {

struct Seg {
    int64_t x, y;
};

inline float clamp_outlier(float v) { return v > 1200.0f ? 1200.0f : (v < 0.0f ? 0.0f : v); }  // jnn.c:19-20,49-83

float mean_f(const float *x, int n) {  // stat.h:17-24: float accumulator, divide by int
    float s = 0;
    for (int i = 0; i < n; ++i) s += x[i];
    return s / n;
}
float stdv_f(const float *x, int n) {  // stat.h:36-44
    const float m = mean_f(x, n);
    float s = 0;
    for (int i = 0; i < n; ++i) s += (x[i] - m) * (x[i] - m);
    return std::sqrt(s / n);
}

// jnnv2(), src/jnn.c:100-180: first low-mean stretch of plausible length in a rolling mean = the adaptor
Seg find_adaptor(const int16_t *raw, int64_t n, int pore) {
    const float std_scale = adaptor_params(pore).std_scale;
    const int seg_dist = kAdSegDist, window = kAdWindow, hi = kAdHi, lo = adaptor_params(pore).lo;
    if (n <= window) return Seg{-1, -1};
    std::vector<float> cur(n);
    for (int64_t i = 0; i < n; ++i) cur[i] = clamp_outlier(static_cast<float>(raw[i]));
    const int m = static_cast<int>(n) - window;
    std::vector<float> t(m);
    float run = 0.0f;  // rolling_window(), jnn.c:22-46
    for (int i = 0; i < window; ++i) run += cur[i];
    t[0] = run / window;
    for (int i = 1; i < m; ++i) {
        run -= cur[i - 1];
        run += cur[i + window - 1];
        t[i] = run / window;
    }
    const float mn = mean_f(t.data(), m), sd = stdv_f(t.data(), m);
    const float bot = mn - (sd * std_scale);
    std::vector<Seg> segs;
    bool begin = false;
    int start = 0, end = 0;
    for (int j = 0; j < m; ++j) {
        const float v = t[j];
        if (v < bot && !begin) {
            start = j;
            begin = true;
        } else if (v < bot) {
            end = j;
        } else if (v > bot && begin) {
            if (!segs.empty() && start - segs.back().y < seg_dist)
                segs.back().y = end;
            else
                segs.push_back(Seg{start, end});
            start = end = 0;
            begin = false;
        }
    }
    Seg p{0, 0};
    for (const Seg &s : segs) {
        const int a = static_cast<int>(s.x), b = static_cast<int>(s.y);
        if (b - a > hi || b - a < lo) continue;
        p.x = a + window / 2 - 1;
        p.y = b + window / 2 - 1;
        break;
    }
    return p;
}

// jnn_core() with JNNV1_R9_POLYA / JNNV1_RNA004_POLYA (identical), src/jnn.c:191-279: first stretch that stays
// inside (bot, top) for >= window samples, tolerating `error` excursions
Seg find_polya(const float *pa, int64_t n, float top, float bot) {
    const int corrector = kPaCorrector, seg_dist = kPaSegDist, window = kPaWindow, error = kPaError;
    const float stall_len = 1.0f;
    std::vector<Seg> segs;
    bool prev = false;
    int err = 0, prev_err = 0, c = 0, w = corrector, start = 0, end = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float a = clamp_outlier(pa[i]);
        if (a < top && a > bot) {
            if (!prev) {
                start = static_cast<int>(i);
                prev = true;
            }
            c++;
            w++;
            if (prev_err) prev_err = 0;
            if (c >= window && c >= w && !(c % w)) err--;
        } else {
            if (prev && err < error) {
                c++;
                err++;
                prev_err++;
                if (c >= window && c >= w && !(c % w)) err--;
            } else if (prev && (c >= window || (segs.empty() && c >= window * stall_len))) {
                end = static_cast<int>(i) - prev_err;
                prev = false;
                if (!segs.empty() && start - segs.back().y < seg_dist)
                    segs.back().y = end;
                else
                    segs.push_back(Seg{start, end});
                c = err = prev_err = 0;
            } else if (prev) {
                prev = false;
                c = err = prev_err = 0;
            }
        }
    }
    return segs.empty() ? Seg{-1, -1} : segs.front();
}

}  // namespace

int64_t auto_start_target(const int16_t *raw, int64_t n, const float *pa, int pore) {
    const Seg ad = find_adaptor(raw, n, pore);
    if (ad.y <= 0) return -1;
    const float m_a = mean_f(pa + ad.x, static_cast<int>(ad.y - ad.x));
    Seg polya = find_polya(pa + ad.y, n - ad.y, m_a + 30 + 20, m_a + 30 - 20);
    if (polya.y <= 0) return -1;
    return polya.y + ad.y;
}

int64_t detect_query_start(const int16_t *raw, int64_t n, const float *pa, const std::vector<sfa_event_t> &ev, int pore) {
    const int64_t target = auto_start_target(raw, n, pa, pore);
    if (target < 0) return -1;
    uint64_t i = 0;
    while (i < ev.size() && ev[i].start < static_cast<uint64_t>(target)) i++;
    return i >= ev.size() ? -1 : static_cast<int64_t>(i);
}

bool select_and_normalise(std::vector<sfa_event_t> &ev, const int16_t *raw, int64_t nraw, const float *pa, int32_t prefix_size,
                          int32_t query_size, uint32_t flag, int pore, int64_t *qstart, int64_t *qend, int *status) {
    // (a caller only comes here with events, and events imply samples: sfa_select_query takes no raw signal with a fixed prefix)
    const bool from_end = (flag & SFA_END) != 0, auto_start = prefix_size < 0 && !from_end;
    const int64_t auto_event = auto_start ? detect_query_start(raw, nraw, pa, ev, pore) : -1;
    const QueryWindow w = query_window(static_cast<int64_t>(ev.size()), 1, prefix_size, query_size, from_end, auto_start, auto_event);
    const int64_t st = *qstart = w.start, en = *qend = w.end;
    *status = w.status;
    if (!w.keep) return false;
    // z-normalise event[st..en).mean in place (src/sigfish.c:483-502), sequential fp32
    const float cnt = static_cast<float>(en - st);
    float mean = 0.0f, var = 0.0f;
    for (int64_t j = st; j < en; ++j) mean += ev[j].mean;
    mean /= cnt;
    for (int64_t j = st; j < en; ++j) {
        const float d = ev[j].mean - mean;
        var += d * d;
    }
    var /= cnt;
    const float sd = static_cast<float>(std::sqrt(static_cast<double>(var)));
    for (int64_t j = st; j < en; ++j) ev[j].mean = (ev[j].mean - mean) / sd;
    return true;
}

}  // namespace sfa
