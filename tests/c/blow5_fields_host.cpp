// blow5_fields_host.cpp -- TEST HARNESS.  The field parser of the device-side BLOW5 reader (sigfish_amd/csrc/blow5_kernels.hpp:
// blow5_parse_fields, the body of blow5_fields_kernel) compiled for the HOST, so that it can run under AddressSanitizer / UBSan
// and beside the host reader (host/blow5.cpp: parse_blow5_record) on the same bytes.  Every payload lies in a heap block of
// exactly its length: a read beyond it is reported.  What is asserted of every case, whatever it was built to show:
//   (a) status 0  =>  n_samples, sig_off, sig_bytes >= 0
//   (b) status 0  =>  sig_off + sig_bytes <= len (compared without a sum that could overflow)
//   (c) status 0  =>  sig_bytes == 2 n_samples (plain int16) or 4 + ceil(n_samples / 4) <= sig_bytes (svb-zd)
//   (d) status 0  =>  parse_blow5_record accepts with the same id, sample count and three doubles, or rejects for the one reason
//                     blow5_svb_kernel reports later: the data stream is not exactly as long as its keys say
//   (e) status -1 and an id that fits the row  =>  parse_blow5_record rejects as well
// and, for the cases written out by hand, the status itself.  usage: blow5_fields_host [mutations] [seed]
#define SFA_HOST_HARNESS
#include "../../sigfish_amd/csrc/blow5_kernels.hpp"
#include "../../sigfish_amd/csrc/host/blow5.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {
using Bytes = std::vector<uint8_t>;
int n_cases = 0, n_failures = 0;

template <typename T> void put(Bytes &b, T v) {
    const uint8_t *q = reinterpret_cast<const uint8_t *>(&v);
    b.insert(b.end(), q, q + sizeof v);
}

const double kDoubles[4] = {8192.0, -243.0, 1437.976685, 4000.0};  // digitisation, offset, range, sampling_rate

// u16 id_len, id, u32 read_group, 4 x f64, u64 length field, then `tail` (signal and whatever follows it)
Bytes payload(uint16_t id_len_field, size_t id_bytes, uint64_t len_field, const Bytes &tail) {
    Bytes b;
    put(b, id_len_field);
    for (size_t i = 0; i < id_bytes; ++i) b.push_back(static_cast<uint8_t>('a' + i % 26));
    put(b, uint32_t(0));
    for (double d : kDoubles) put(b, d);
    put(b, len_field);
    b.insert(b.end(), tail.begin(), tail.end());
    return b;
}
int64_t fixed_of(size_t id_bytes) { return 2 + static_cast<int64_t>(id_bytes) + 4 + 32 + 8; }

// a canonical svb-zd stream of n samples (value i needs 1 + (i + salt) % 4 bytes), `count_field` in front
Bytes svb_stream(uint32_t count_field, uint32_t n, unsigned salt = 0) {
    Bytes keys((n + 3) / 4, 0), data;
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned code = (i + salt) % 4;
        keys[i / 4] |= static_cast<uint8_t>(code << (2 * (i % 4)));
        for (unsigned t = 0; t <= code; ++t) data.push_back(static_cast<uint8_t>(2 * (i + t)));  // (even low byte: small positive deltas)
    }
    Bytes s;
    put(s, count_field);
    s.insert(s.end(), keys.begin(), keys.end());
    s.insert(s.end(), data.begin(), data.end());
    return s;
}

void failure(const char *label, const char *what, long long a = 0, long long b = 0) {
    if (++n_failures <= 40) printf("FAIL %s: %s (%lld, %lld)\n", label, what, a, b);
}

// `expect`: the status a hand-written case must get (0, -1), or 1: whatever the parser says, the invariants decide
void check(const char *label, const Bytes &pl, int svb, int expect) {
    ++n_cases;
    const int64_t len = static_cast<int64_t>(pl.size());
    uint8_t *p = new uint8_t[pl.size()];  // exactly len bytes (none at all for an empty payload)
    if (len) memcpy(p, pl.data(), pl.size());
    uint8_t *h = new uint8_t[sfa::kBlow5HeadBytes];
    memset(h, 0xaa, sfa::kBlow5HeadBytes);
    sfa::blow5_parse_fields(p, len, svb, h);
    int32_t status, id_len;
    int64_t ns, off, bytes;
    double f[3];
    memcpy(&status, h + sfa::kHeadStatus, 4);
    memcpy(&id_len, h + sfa::kHeadIdLen, 4);
    memcpy(&ns, h + sfa::kHeadSamples, 8);
    memcpy(f, h + sfa::kHeadScaling, 24);
    memcpy(&off, h + sfa::kHeadSigOff, 8);
    memcpy(&bytes, h + sfa::kHeadSigBytes, 8);
    if (status != 0 && status != -1) failure(label, "status is neither 0 nor -1", status);
    if (expect != 1 && status != expect) failure(label, "status differs from the expected one: got, expected", status, expect);
    sfa::Blow5Record rec;
    std::string err;
    const bool host_ok = sfa::parse_blow5_record(p, pl.size(), 0, svb, &rec, &err);
    if (status == 0) {
        bool sound = true;
        if (ns < 0 || off < 0 || bytes < 0) failure(label, "(a) negative field: n_samples, sig_bytes", ns, bytes), sound = false;
        if (sound && (off > len || bytes > len - off)) failure(label, "(b) signal beyond the payload: sig_bytes, len - sig_off", bytes, len - off), sound = false;
        if (sound && !svb && (ns > INT64_MAX / 2 || bytes != 2 * ns)) failure(label, "(c) sig_bytes != 2 n_samples", bytes, ns), sound = false;
        if (sound && svb && (bytes < 4 || (ns + 3) / 4 > bytes - 4)) failure(label, "(c) keys beyond sig_bytes", bytes, ns), sound = false;
        if (sound && (id_len < 0 || id_len > sfa::kBlow5IdMax)) failure(label, "id_len outside the row", id_len), sound = false;
        if (sound && host_ok) {
            if (rec.read_id.size() != static_cast<size_t>(id_len) || memcmp(rec.read_id.data(), h + sfa::kHeadId, id_len) != 0) failure(label, "(d) read id differs");
            if (static_cast<int64_t>(rec.raw.size()) != ns) failure(label, "(d) sample count differs: device, host", ns, static_cast<long long>(rec.raw.size()));
            const double hf[3] = {rec.digitisation, rec.offset, rec.range};
            if (memcmp(hf, f, 24) != 0) failure(label, "(d) digitisation / offset / range differ");
        }
        if (sound) {  // the host reader may reject only what blow5_svb_kernel flags: keys that add up to another length than the data has
            bool stream_exact = true;
            if (svb) {
                const uint8_t *keys = p + off + 4;
                int64_t need = 0;
                for (int64_t i = 0; i < ns; ++i) need += 1 + ((keys[i >> 2] >> ((i & 3) * 2)) & 3);
                stream_exact = need == bytes - 4 - (ns + 3) / 4;
            }
            if (!host_ok && stream_exact) failure(label, "(d) the host reader rejects what the device parser accepts");
            if (host_ok && !stream_exact) failure(label, "harness: the host reader accepts a stream of the wrong length");
        }
    } else if (status == -1) {
        const bool id_fits = len < 2 || (p[0] | (p[1] << 8)) <= sfa::kBlow5IdMax;
        if (id_fits && host_ok) failure(label, "(e) the host reader accepts what the device parser rejects: host samples", static_cast<long long>(rec.raw.size()));
    }
    delete[] p;
    delete[] h;
}

Bytes cut(Bytes b, int64_t len) {
    b.resize(static_cast<size_t>(len), 0x5a);
    return b;
}
}  // namespace

int main(int argc, char **argv) {
    const int mutations = argc > 1 ? atoi(argv[1]) : 4000;
    srand(argc > 2 ? atoi(argv[2]) : 1);
    const uint64_t P31 = uint64_t(1) << 31, P62 = uint64_t(1) << 62, P63 = uint64_t(1) << 63;
    const size_t ID = 5;
    const int64_t fixed = fixed_of(ID);
    char label[160];

    // ---- payload lengths around the fixed fields, both methods ----
    for (int svb = 0; svb < 2; ++svb) {
        // plain: two samples announced and present; svb-zd: an empty stream (l = 4, count 0), the least the method allows
        const Bytes whole = svb ? payload(ID, ID, 4, svb_stream(0, 0)) : payload(ID, ID, 2, Bytes{1, 0, 2, 0});
        const int64_t lens[6] = {0, 1, fixed - 1, fixed, fixed + 3, fixed + 4};
        for (int64_t len : lens) {
            snprintf(label, sizeof label, "svb=%d len=%lld (fixed=%lld)", svb, static_cast<long long>(len), static_cast<long long>(fixed));
            check(label, cut(whole, len), svb, len >= fixed + 4 ? 0 : -1);
        }
        // ... and with nothing announced: a plain record of no samples is complete at `fixed`, an svb-zd one is not (l < 4)
        const Bytes none = payload(ID, ID, 0, Bytes{});
        for (int64_t len : lens) {
            snprintf(label, sizeof label, "svb=%d len=%lld length field 0", svb, static_cast<long long>(len));
            check(label, cut(none, len), svb, !svb && len >= fixed ? 0 : -1);
        }
    }

    // ---- id lengths ----
    for (int svb = 0; svb < 2; ++svb) {
        const int ids[7] = {0, 1, 127, 128, sfa::kBlow5IdMax, sfa::kBlow5IdMax + 1, 65535};
        for (int id : ids) {
            const Bytes sig = svb ? svb_stream(7, 7) : Bytes(14, 3);
            snprintf(label, sizeof label, "svb=%d id_len=%d", svb, id);
            check(label, payload(static_cast<uint16_t>(id), id, svb ? sig.size() : 7, sig), svb, id <= sfa::kBlow5IdMax ? 0 : -1);
            snprintf(label, sizeof label, "svb=%d id_len=%d announced, 3 id bytes present", svb, id);
            check(label, payload(static_cast<uint16_t>(id), 3, svb ? sig.size() : 7, sig), svb, 1);
            snprintf(label, sizeof label, "svb=%d id_len=%d announced, payload ends inside the id", svb, id);
            check(label, cut(payload(static_cast<uint16_t>(id), id, 0, Bytes{}), 2 + id / 2), svb, id == 0 ? 1 : -1);
        }
    }

    // ---- plain int16: the length field ----
    {
        const int S = 10;
        const Bytes sig(2 * S, 7);
        const struct { uint64_t field; int expect; const char *name; } cases[] = {
            {0, 0, "0"}, {S, 0, "exactly what fits"}, {S + 1, -1, "one more than fits"}, {P31, -1, "2^31"}, {P62, -1, "2^62"},
            {P62 + 1, -1, "2^62+1"}, {P63 - 1, -1, "2^63-1"}, {P63, -1, "2^63"}, {~uint64_t(0), -1, "2^64-1"}};
        for (const auto &c : cases) {
            snprintf(label, sizeof label, "plain length field %s", c.name);
            check(label, payload(ID, ID, c.field, sig), 0, c.expect);
            snprintf(label, sizeof label, "plain length field %s, odd byte behind the samples", c.name);
            Bytes odd(sig);
            odd.push_back(9);
            check(label, payload(ID, ID, c.field, odd), 0, c.expect);
            snprintf(label, sizeof label, "plain length field %s, no signal bytes at all", c.name);
            check(label, payload(ID, ID, c.field, Bytes{}), 0, c.field == 0 ? 0 : -1);
        }
        check("plain, auxiliary bytes behind the signal", payload(ID, ID, S - 3, sig), 0, 0);
    }

    // ---- svb-zd: the byte count l ----
    {
        const Bytes st = svb_stream(9, 9);
        const uint64_t exact = st.size();
        const struct { uint64_t l; int expect; const char *name; } cases[] = {
            {0, -1, "0"}, {3, -1, "3"}, {exact, 0, "exact"}, {exact + 1, -1, "one beyond len"}, {P63 - 1, -1, "2^63-1"}, {P63, -1, "2^63"},
            {~uint64_t(0), -1, "2^64-1"}, {P62, -1, "2^62"}, {~uint64_t(0) - static_cast<uint64_t>(fixed) + 1, -1, "2^64-fixed"},
            {P63 - static_cast<uint64_t>(fixed), -1, "2^63-fixed"}, {P63 - static_cast<uint64_t>(fixed) - 1, -1, "2^63-fixed-1"}};
        for (const auto &c : cases) {
            snprintf(label, sizeof label, "svb l=%s", c.name);
            check(label, payload(ID, ID, c.l, st), 1, c.expect);
            snprintf(label, sizeof label, "svb l=%s, payload ends at the fixed fields", c.name);
            check(label, payload(ID, ID, c.l, Bytes{}), 1, -1);
            snprintf(label, sizeof label, "svb l=%s, three bytes behind the fixed fields", c.name);
            check(label, payload(ID, ID, c.l, Bytes{9, 0, 0}), 1, -1);
        }
        check("svb l=4 with count 0", payload(ID, ID, 4, svb_stream(0, 0)), 1, 0);
        check("svb l=4 with count 1 (no room for its key)", payload(ID, ID, 4, svb_stream(1, 0)), 1, -1);
        check("svb count 0, auxiliary bytes behind the signal", payload(ID, ID, 4, svb_stream(0, 9)), 1, 0);
        check("svb exact, auxiliary bytes behind the signal", [&] { Bytes t(st); t.insert(t.end(), 11, 0xee); return payload(ID, ID, exact, t); }(), 1, 0);
        check("svb one surplus data byte inside l", [&] { Bytes t(st); t.push_back(0); return payload(ID, ID, exact + 1, t); }(), 1, 0);
        check("svb one data byte short", [&] { Bytes t(st); t.pop_back(); return payload(ID, ID, exact - 1, t); }(), 1, 0);
        // a count whose keys just fit into l (the fields are in order; the data stream is then empty: the kernel's business) and
        // just do not; 2^31 is the largest count the row takes, far beyond these keys either way
        for (uint32_t n : {1u, 4u, 5u, 255u, 256u, 257u}) {
            const uint64_t nk = (n + 3) / 4;
            Bytes t;
            put(t, n);
            t.insert(t.end(), nk, 0);
            snprintf(label, sizeof label, "svb count %u, l = 4 + keys", n);
            check(label, payload(ID, ID, 4 + nk, t), 1, 0);
            snprintf(label, sizeof label, "svb count %u, l = 4 + keys - 1", n);
            check(label, payload(ID, ID, 4 + nk - 1, t), 1, -1);
        }
        for (uint64_t n : {P31, P31 + 1, uint64_t(0xffffffffu)}) {
            snprintf(label, sizeof label, "svb count %llu in a stream of %llu bytes", static_cast<unsigned long long>(n), static_cast<unsigned long long>(exact));
            Bytes t(st);
            const uint32_t n32 = static_cast<uint32_t>(n);
            memcpy(t.data(), &n32, 4);
            check(label, payload(ID, ID, exact, t), 1, -1);
        }
    }

    // ---- seeded random mutations of valid payloads ----
    const uint64_t edges[] = {0, 1, 2, 3, 4, 5, P31 - 1, P31, P31 + 1, P62 - 1, P62, P62 + 1, P63 - 1, P63, P63 + 1, ~uint64_t(0), ~uint64_t(0) - 1};
    for (int it = 0; it < mutations; ++it) {
        const int svb = rand() & 1;
        const size_t id = rand() % 4 == 0 ? static_cast<size_t>(sfa::kBlow5IdMax - 2 + rand() % 5) : static_cast<size_t>(rand() % 40);
        const uint32_t n = rand() % 3 == 0 ? rand() % 6 : rand() % 700;
        Bytes sig = svb ? svb_stream(n, n, rand()) : Bytes(2 * n);
        for (uint8_t &b : sig)
            if (!svb) b = static_cast<uint8_t>(rand());
        const uint64_t field = svb ? sig.size() : n;
        if (rand() & 1) sig.insert(sig.end(), rand() % 20, 0xee);  // auxiliary fields
        Bytes pl = payload(static_cast<uint16_t>(id), id, field, sig);
        const size_t at_len = 2 + id + 4 + 32;  // where the length field lies
        const int kind = rand() % 8;
        int expect = 1;
        if (kind == 0) {  // untouched
            expect = id <= static_cast<size_t>(sfa::kBlow5IdMax) ? 0 : -1;
        } else if (kind == 1) {  // an edge value, or one near the true one, in the length field
            uint64_t v = rand() & 1 ? edges[rand() % (sizeof edges / sizeof edges[0])] : field + static_cast<uint64_t>(rand() % 9 - 4);
            if (rand() % 4 == 0) v = (static_cast<uint64_t>(rand()) << 33) ^ (static_cast<uint64_t>(rand()) << 11) ^ static_cast<uint64_t>(rand());
            memcpy(pl.data() + at_len, &v, 8);
        } else if (kind == 2) {  // truncated anywhere
            pl.resize(rand() % (pl.size() + 1));
        } else if (kind == 3) {  // truncated near the end of the fixed fields
            pl.resize(std::min(pl.size(), at_len + static_cast<size_t>(rand() % 16)));
        } else if (kind == 4) {  // a few bytes flipped anywhere
            for (int k = 1 + rand() % 4; k > 0; --k) pl[rand() % pl.size()] ^= static_cast<uint8_t>(1 << (rand() % 8));
        } else if (kind == 5) {  // the id length field
            const uint16_t v = rand() & 1 ? static_cast<uint16_t>(rand()) : static_cast<uint16_t>(id + rand() % 5 - 2);
            memcpy(pl.data(), &v, 2);
        } else if (kind == 6 && svb && pl.size() >= at_len + 12) {  // the sample count of an svb-zd stream
            const uint32_t v = rand() & 1 ? static_cast<uint32_t>(edges[rand() % 9]) : n + static_cast<uint32_t>(rand() % 9 - 4);
            memcpy(pl.data() + at_len + 8, &v, 4);
        } else {  // random bytes behind the id
            for (size_t i = 2 + id; i < pl.size(); ++i)
                if (rand() % 3 == 0) pl[i] = static_cast<uint8_t>(rand());
        }
        snprintf(label, sizeof label, "mutation %d (svb=%d id=%zu n=%u kind=%d, %zu bytes)", it, svb, id, n, kind, pl.size());
        check(label, pl, svb, expect);
    }
    printf("%d cases, %d failures\n", n_cases, n_failures);
    return n_failures != 0;
}
