// sfa_auto_start_target (host/events.cpp: the target of a raw session's automatic query start) under ASan + UBSan, host code only:
// prefixes of lengths 0, 1, 2000, 2001 and every length around the sample at which the poly-A stretch of a synthetic read closes.
// The target of a prefix must be -1 or lie inside the prefix, a prefix of at most 2000 samples has none, the whole read has one,
// and it is the sample sfa_detect_query_start's event walk starts from.  Built and run by tests/test_autostart_stream_cpu.py.
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
static double gauss() {
    double s = 0;
    for (int i = 0; i < 12; ++i) s += uni();
    return s - 6.0;
}

static const double kDig = 2048.0, kOff = -240.0, kRange = 548.7882690429688;

static void stretch(std::vector<int16_t> &raw, int n, double level, double level_sd, double noise) {
    while (n > 0) {
        const double lv = level + level_sd * gauss();
        const int dwell = 5 + static_cast<int>(rnd() % 35);
        for (int k = 0; k < dwell && n > 0; ++k, --n) raw.push_back(static_cast<int16_t>((lv + noise * gauss()) * kDig / kRange - kOff));
    }
}

int main() {
    int failures = 0;
    for (int pore = 0; pore <= 2; pore += 2) {
        // leader, adaptor (low), poly-A plateau 30 pA above it, transcript
        std::vector<int16_t> raw;
        stretch(raw, 1500, 112.0, 3.0, 2.0);
        stretch(raw, 6000, 60.0, 0.0, 2.0);
        const int polya_from = static_cast<int>(raw.size());
        stretch(raw, 900, 90.0, 0.0, 1.5);
        const int polya_to = static_cast<int>(raw.size());
        stretch(raw, 9000, 128.0, 6.0, 2.0);  // transcript levels well above the poly-A band (adaptor mean + 30 +- 20)
        const int64_t n = static_cast<int64_t>(raw.size());
        const int64_t whole = sfa_auto_start_target(raw.data(), n, kDig, kOff, kRange, pore);
        if (whole < polya_from || whole > polya_to + 400) {
            printf("pore %d: the whole read's target %lld is not at the end of the poly-A stretch [%d, %d)\n", pore, static_cast<long long>(whole), polya_from, polya_to);
            ++failures;
        }
        std::vector<int64_t> lens = {0, 1, 2000, 2001, n};
        for (int64_t l = polya_to - 40; l <= polya_to + 600; ++l) lens.push_back(l);
        for (int64_t l = whole - 3; l <= whole + 3; ++l) lens.push_back(l);
        int64_t found = 0;
        for (int64_t l : lens) {
            // an exact-size copy: a read behind the prefix's end is the sanitizer's
            std::vector<int16_t> pre(raw.begin(), raw.begin() + l);
            const int64_t t = sfa_auto_start_target(l ? pre.data() : nullptr, l, kDig, kOff, kRange, pore);
            if (t < -1 || t >= l || (l <= 2000 && t != -1)) {
                printf("pore %d: prefix %lld gives target %lld\n", pore, static_cast<long long>(l), static_cast<long long>(t));
                ++failures;
            }
            found += t >= 0;
        }
        if (!found) {
            printf("pore %d: no prefix around the closing poly-A gave a target\n", pore);
            ++failures;
        }
        // the event walk of sfa_detect_query_start starts from the target
        std::vector<sfa_event_t> ev(static_cast<size_t>(n / 2 + 16));
        memset(ev.data(), 0, sizeof(sfa_event_t) * ev.size());
        const int64_t nev = sfa_detect_events(raw.data(), n, kDig, kOff, kRange, 1, ev.data(), static_cast<int64_t>(ev.size()));
        const int64_t st = sfa_detect_query_start(raw.data(), n, kDig, kOff, kRange, ev.data(), nev, pore);
        int64_t want = -1;
        for (int64_t i = 0; i < nev && whole >= 0; ++i)
            if (ev[i].start >= static_cast<uint64_t>(whole)) {
                want = i;
                break;
            }
        if (st != want) {
            printf("pore %d: sfa_detect_query_start %lld, the first event behind the target %lld\n", pore, static_cast<long long>(st), static_cast<long long>(want));
            ++failures;
        }
        printf("pore %d: %zu prefixes, %lld with a target, whole read %lld, start event %lld\n", pore, lens.size(), static_cast<long long>(found), static_cast<long long>(whole),
               static_cast<long long>(st));
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
