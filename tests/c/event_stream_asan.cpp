// The streaming event detector (sfa_event_stream_*, host/events.cpp) under ASan + UBSan, host code only: three synthetic signals
// pushed through several chunk schedules; everything push and finish return must be the table of sfa_detect_events over the
// whole signal, byte for byte.  Built and run by tests/test_event_stream_asan.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/sigfish_amd.h"

extern "C" void sfa_set_error_(const char *) {}  // (sfa_host.cpp reports through the library's error slot)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return static_cast<uint32_t>((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
static double uni() { return (rnd() + 0.5) / 4294967296.0; }
static double gauss() {  // sum of 12 uniforms
    double s = 0;
    for (int i = 0; i < 12; ++i) s += uni();
    return s - 6.0;
}

static const double kDig = 8192.0, kOff = 6.0, kRange = 1467.61;

// piecewise-constant levels ~N(90, 12) pA, dwell 6..12 samples, noise sd 1.5, as ADC counts
static std::vector<int16_t> make_signal(int n) {
    std::vector<int16_t> raw;
    while (static_cast<int>(raw.size()) < n) {
        const double level = 90.0 + 12.0 * gauss();
        const int dwell = 6 + static_cast<int>(rnd() % 7);
        for (int k = 0; k < dwell && static_cast<int>(raw.size()) < n; ++k) {
            const double pa = level + 1.5 * gauss();
            raw.push_back(static_cast<int16_t>(pa * kDig / kRange - kOff));
        }
    }
    return raw;
}

static int failures = 0;

static void run(const std::vector<int16_t> &raw, int rna, const std::vector<int64_t> &chunks, const char *what) {
    const int64_t n = static_cast<int64_t>(raw.size());
    std::vector<sfa_event_t> want(static_cast<size_t>(n / 2 + 16));
    memset(want.data(), 0, sizeof(sfa_event_t) * want.size());
    const int64_t nw = sfa_detect_events(raw.data(), n, kDig, kOff, kRange, rna, want.data(), static_cast<int64_t>(want.size()));
    std::vector<sfa_event_t> got;
    sfa_event_stream_t *es = sfa_event_stream_create(kDig, kOff, kRange, rna);
    int64_t at = 0;
    size_t ci = 0;
    std::vector<sfa_event_t> buf(4);
    auto deliver = [&](bool fin, const int16_t *p, int64_t len) {
        for (;;) {
            memset(buf.data(), 0, sizeof(sfa_event_t) * buf.size());  // (padding bytes compare equal)
            const int64_t k = fin ? sfa_event_stream_finish(es, buf.data(), static_cast<int64_t>(buf.size()))
                                  : sfa_event_stream_push(es, p, len, buf.data(), static_cast<int64_t>(buf.size()));
            if (k < 0) {
                ++failures;
                printf("%s: call failed (%lld)\n", what, static_cast<long long>(k));
                return;
            }
            if (k > static_cast<int64_t>(buf.size())) {  // nothing was consumed: a larger buffer, the same samples
                buf.resize(static_cast<size_t>(k));
                continue;
            }
            got.insert(got.end(), buf.begin(), buf.begin() + k);
            return;
        }
    };
    while (at < n) {
        int64_t len = chunks.empty() ? n : chunks[ci++ % chunks.size()];
        if (len > n - at) len = n - at;
        deliver(false, raw.data() + at, len);
        at += len;
    }
    deliver(true, nullptr, 0);
    if (sfa_event_stream_push(es, raw.data(), 1, buf.data(), 1) != SFA_EINVAL) ++failures;  // samples after finish
    sfa_event_stream_destroy(es);
    bool same = static_cast<int64_t>(got.size()) == nw;
    for (int64_t e = 0; same && e < nw; ++e) {
        same = got[e].start == want[e].start && !memcmp(&got[e].length, &want[e].length, 4) && !memcmp(&got[e].mean, &want[e].mean, 4) &&
               !memcmp(&got[e].stdv, &want[e].stdv, 4);
    }
    if (!same) {
        ++failures;
        printf("%s: %lld events, the batch routine has %lld\n", what, static_cast<long long>(got.size()), static_cast<long long>(nw));
    }
}

int main() {
    const int sizes[3] = {4000, 1777, 600};
    int runs = 0;
    for (int si = 0; si < 3; ++si) {
        const std::vector<int16_t> raw = make_signal(sizes[si]);
        for (int rna = 0; rna < 2; ++rna) {
            const int64_t wl = rna ? 14 : 6;
            std::vector<int64_t> random_chunks;
            for (int i = 0; i < 97; ++i) random_chunks.push_back(1 + rnd() % 400);
            const std::vector<std::vector<int64_t>> schedules = {
                {},                                         // the whole read at once
                random_chunks,                              // 1 .. 400
                {0, 37, 0, 0, 250, 0},                      // with empty chunks
                {2 * wl - 1, 1, 1, 300},                    // cuts at 2 w_long - 1, 2 w_long, 2 w_long + 1
            };
            for (const auto &sc : schedules) {
                run(raw, rna, sc, "schedule");
                ++runs;
            }
            if (sizes[si] <= 600) {
                run(raw, rna, {1}, "1-sample chunks");
                ++runs;
            }
        }
    }
    // shorter than 2 w_long, constant
    for (int rna = 0; rna < 2; ++rna) {
        run(make_signal(2 * (rna ? 14 : 6) - 1), rna, {5}, "short");
        run(std::vector<int16_t>(500, 700), rna, {64}, "constant");
        runs += 2;
    }
    // null arguments
    sfa_event_t e;
    sfa_event_stream_t *es = sfa_event_stream_create(kDig, kOff, kRange, 0);
    const int16_t one = 1;
    if (sfa_event_stream_push(nullptr, &one, 1, &e, 1) != SFA_EINVAL) ++failures;
    if (sfa_event_stream_push(es, nullptr, 1, &e, 1) != SFA_EINVAL) ++failures;
    if (sfa_event_stream_push(es, &one, 1, nullptr, 1) != SFA_EINVAL) ++failures;
    if (sfa_event_stream_finish(nullptr, &e, 1) != SFA_EINVAL) ++failures;
    sfa_event_stream_destroy(es);
    sfa_event_stream_destroy(nullptr);
    printf("%d runs, %d failures\n", runs, failures);
    return failures ? 1 : 0;
}
