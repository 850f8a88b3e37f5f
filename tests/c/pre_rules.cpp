// pre_rules.cpp -- the host rules in front of the DP (sigfish_amd/csrc/pre_rules.hpp) as a stand-alone program: built from that
// header alone with g++ -Wall -Werror, once more under ASan + UBSan, and driven by tests/test_pre_rules_cpu.py.  It prints the
// tables and query_window() over a grid that crosses every branch of the rule:
//   det RNA W1 W2 THR1 THR2 PEAK_HEIGHT            adaptor PORE LO STD_SCALE            cap LEN CAPACITY
//   scale DIGITISATION OFFSET RANGE -> offset and unit as the bits of their floats
//   win N_EVENTS N_SAMPLES PREFIX QUERY FROM_END AUTO AUTO_EVENT -> START END STATUS KEEP
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "pre_rules.hpp"

static void win(long long n_events, long long n_samples, int prefix, int query, bool from_end, bool auto_start, long long auto_event) {
    const sfa::QueryWindow w = sfa::query_window(n_events, n_samples, prefix, query, from_end, auto_start, auto_event);
    printf("win %lld %lld %d %d %d %d %lld -> %lld %lld %d %d\n", n_events, n_samples, prefix, query, from_end ? 1 : 0, auto_start ? 1 : 0, auto_event,
           static_cast<long long>(w.start), static_cast<long long>(w.end), w.status, w.keep ? 1 : 0);
}

static unsigned bits(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

int main() {
    for (int rna = 0; rna < 2; ++rna) {
        const sfa::DetectorParams p = sfa::detector_params(rna != 0);
        printf("det %d %d %d %.9g %.9g %.9g\n", rna, p.w1, p.w2, p.thr1, p.thr2, p.peak_height);
    }
    for (int pore = 0; pore < 3; ++pore) printf("adaptor %d %d %.9g\n", pore, sfa::adaptor_params(pore).lo, sfa::adaptor_params(pore).std_scale);
    for (long long len : {0LL, 1LL, 4000LL, 1LL << 31}) printf("cap %lld %lld\n", len, static_cast<long long>(sfa::event_capacity(len)));
    const double scalings[][3] = {{8192.0, 6.0, 1467.61}, {2048.0, -243.0, 748.5801}, {8192.0, 0.1, 1e-3}};
    for (const double *s : scalings) {
        const sfa::RawScale r = sfa::raw_scale(s[0], s[1], s[2]);
        printf("scale %.17g %.17g %.17g -> %08x %08x\n", s[0], s[1], s[2], bits(r.offset), bits(r.unit));
    }
    printf("status %d %d %d fallback %d\n", sfa::kQueryShort, sfa::kQueryDropped, sfa::kQueryAutoFailed, sfa::kAutoFallback);
    long long counts[88];
    int n_counts = 0;
    for (long long n = 0; n <= 80; ++n) counts[n_counts++] = n;
    for (long long n : {249LL, 250LL, 251LL, 299LL, 300LL, 301LL, 2048LL}) counts[n_counts++] = n;
    for (int k = 0; k < n_counts; ++k) {
        const long long n = counts[k];
        for (int query : {1, 25, 250}) {
            for (int prefix : {0, 1, 50, 60})
                for (int from_end = 0; from_end < 2; ++from_end) {
                    win(n, 4000, prefix, query, from_end != 0, false, -1);
                    win(n, 0, prefix, query, from_end != 0, false, -1);  // events cannot be without samples; the rule says what then
                }
            for (long long auto_event : {-1LL, 0LL, 10LL, 55LL, n}) win(n, 4000, -1, query, false, true, auto_event);
        }
    }
    return 0;
}
